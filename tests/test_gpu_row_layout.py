"""Every block of the expect-row layout in ONE call, so that a block offset that is wrong by one block lands in a neighbour's rows
(csrc/plan.hpp: ExpectRows; solver._Call.expect_rows): forward values, backward with a one-hot cotangent on one row inside each
block, and the tangent sweep.  The tests of each kernel family request one or two blocks at a time; no other test requests diagonal,
Pauli, overlap and RDM rows together for forward, backward and tangent, nor all five kinds of density-matrix rows.

Ket case: 4 qubits, B = 2, 3 save points, KRYLOV_SE, the seeded problem of tests/test_gpu_tangent_matrix.py (random_terms(local=True));
two diagonal rows, two Pauli rows, one overlap (two rows), RDMs with m = 1 and m = 2 (8 + 32 rows).  Values and gradients against
the dense oracle (R.krylov_map_dense, autograd), tangents against tests.helpers.tangent_dense_reference.

Density-matrix case: 2 atoms, B = 1, dephasing, the recorded oracle case of tests/dm_tangent_reference.py cut to its first 3 save
points (the map of an interval does not depend on later ones): two diagonal rows, two Pauli rows, two fidelities, the purity and one
reduced density matrix through mesolve(store_states=False); the recorded directional derivatives are the reference of the one-hot
gradients (<gradient, direction d> = der[d, row, k]), the dense Lindblad oracle of tests/test_gpu_dm_rdm.py that of the RDM block.
The same rows without the RDM through mesolve_tangent, two directions.

Tolerances are those of the tests that cover each kernel family; every use names its source line."""
import pytest
import torch

from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd.lindblad import mesolve, mesolve_tangent
from pulser_diff_amd.observables import ReducedDensityMatrix, StateOverlap, pack_overlaps, reduced_density_matrix
from pulser_diff_amd.solver import SolverType, evolve, evolve_tangent, split_observables
from tests.dm_tangent_reference import NOISE, ZERO_DIRECTION, h_max
from tests.helpers import tangent_dense_reference, tangent_rows_reference, to_native
from tests.test_gpu_dm_tangent import TANGENT_RTOL, VALUE_ATOL as DM_VALUE_ATOL, _oracle_case
from tests.test_gpu_master_equation_sizes import _ham_like, _noise_model
from tests.test_gpu_rdm_tangent import ORACLE_RTOL, VALUE_ATOL, _native_rdms, _partial, _reference_rdms
from tests.test_gpu_tangent import observable_set
from tests.test_gpu_tangent_matrix import TSAVE_9, _inputs, _problem, _terms_with_tables

pytestmark = pytest.mark.gpu

N, BATCH, N_DIR = 4, 2, 2
SUBSYSTEMS = [(3,), (2, 0)]  # m = 1 and m = 2 (scrambled: the highest and the lowest index bit)
N_REAL = 6                   # diagonal rows 0-1, Pauli rows 2-3, overlap rows 4-5 (Re, Im); the RDM block: rows 6-13 and 14-45


def _ket_rows(prob):
    return prob["diags"][:2], observable_set(N)[:2], prob["targets_traj"][:1]


def _ket_call(prob, dev, store_states=False):
    diag, pauli, targets = _ket_rows(prob)
    _, _, _, spec = to_native(prob["terms"], dev, SolverType.KRYLOV_SE, store_states=store_states)
    spec.pauli = pauli
    spec.overlaps = pack_overlaps([StateOverlap(t) for t in targets], 2 ** N, BATCH, dev)
    spec.rdms = [ReducedDensityMatrix(qs) for qs in SUBSYSTEMS]
    return spec, diag.to(dev)


def _ket_weights(prob):
    """What a row's value error is measured against (tests/test_gpu_tangent_matrix.py:165): max |diagonal|, sum |w_s|, 1 for a
    normalised target."""
    diag, pauli, targets = _ket_rows(prob)
    return torch.tensor([float(d.abs().max()) for d in diag] + [sum(abs(w) for w, _, _ in p.terms) for p in pauli] + [1.0] * (2 * len(targets)),
                        dtype=torch.float64)


def _picked(real_rows, rdms):
    """One scalar inside each of the four blocks: diagonal row 1, Pauli row 1, the Im row of the overlap, Re of an off-diagonal entry
    of the m = 2 matrix — each at its own save point and trajectory."""
    return {"diagonal": real_rows[1, 2, 1], "pauli": real_rows[3, 2, 0], "overlap": real_rows[5, 1, 1], "rdm": rdms[1][2, 1, 1, 2].real}


def test_ket_rows_values_and_one_hot_gradients_of_every_block(cuda_device):
    dev = cuda_device
    prob = _problem(N, BATCH, 1, N_DIR)
    diag, pauli, targets = _ket_rows(prob)
    tsave = torch.tensor(TSAVE_9, dtype=torch.float64)
    # the oracle: dense states, the rows in float64 torch, autograd
    o_amp, o_det = prob["amp"][0].clone().requires_grad_(True), prob["det"][0].clone().requires_grad_(True)
    states = R.krylov_map_dense(_terms_with_tables(prob["terms"], o_amp, o_det), prob["psi0"].T.contiguous(), tsave)
    want_real = tangent_rows_reference(states, torch.zeros(len(tsave), 1, 2 ** N, BATCH, dtype=torch.complex128), diag, pauli, targets)[0]
    want_rdms = [_partial(states, states, qs, N) for qs in SUBSYSTEMS]
    # native
    spec, diag_dev = _ket_call(prob, dev)
    amp, det = prob["amp"].to(dev).requires_grad_(True), prob["det"].to(dev).requires_grad_(True)
    _, expect = evolve(amp, det, prob["u"].to(dev), tsave, prob["psi0"].to(dev), spec, diag_dev)
    assert tuple(expect.shape) == (N_REAL + 8 + 32, len(tsave), BATCH)
    got_real, got_ov, got_rdms = split_observables(expect, 1, spec.rdms)
    got_real = torch.cat([got_real, got_ov.real, got_ov.imag])  # the native order of the real rows
    val_err = (got_real.detach().cpu() - want_real.detach()).abs().amax(dim=(1, 2)) / _ket_weights(prob)
    print(f"ROW-LAYOUT ket values: largest error / row weight per row {[f'{float(e):.1e}' for e in val_err]}")
    assert float(want_real.detach().abs().max()) > 1e-2  # tests/test_gpu_tangent_matrix.py:180
    assert float(val_err.max()) <= VALUE_ATOL  # tests/test_gpu_rdm_tangent.py:47 (tests/test_gpu_tangent_matrix.py:53,181)
    for qs, got, want in zip(SUBSYSTEMS, got_rdms, want_rdms):
        err = float((got.detach().cpu() - want.detach()).abs().max())
        print(f"ROW-LAYOUT ket values: A={qs} max error {err:.2e}")
        assert err <= VALUE_ATOL  # tests/test_gpu_rdm_tangent.py:47,136
    got_picked, want_picked = _picked(got_real, got_rdms), _picked(want_real, want_rdms)
    for block in got_picked:  # four backward calls, one row each
        g_amp, g_det = torch.autograd.grad(got_picked[block], [amp, det], retain_graph=True)
        w_amp, w_det = torch.autograd.grad(want_picked[block], [o_amp, o_det], retain_graph=True)
        for name, got, want in (("amp", g_amp[0].cpu(), w_amp), ("det", g_det[0].cpu(), w_det)):
            scale, err = float(want.abs().max()), float((got - want).abs().max())
            print(f"ROW-LAYOUT ket gradient of the {block} row w.r.t. {name}: largest entry {scale:.3e}, max error {err:.3e}")
            assert scale > 1e-4  # nothing passes on zeros
            assert err <= ORACLE_RTOL * scale  # tests/test_gpu_rdm_tangent.py:42 (1e-8 of the largest entry: tests/test_gpu_rdm_observables.py:26)


def test_ket_rows_tangents_of_every_block(cuda_device):
    dev = cuda_device
    prob = _problem(N, BATCH, 1, N_DIR)
    diag, pauli, targets = _ket_rows(prob)
    tsave = torch.tensor(TSAVE_9, dtype=torch.float64)
    d_amp, d_det, d_u, d_psi = _inputs(prob, "adup", 0, N_DIR)
    ref = tangent_dense_reference(prob["ref_terms"], d_amp[:, 0], d_det[:, 0], d_u, prob["psi0"].T.contiguous(), d_psi.permute(0, 2, 1).contiguous(),
                                  tsave, SolverType.KRYLOV_SE)
    want_val, want_der = tangent_rows_reference(ref[0], ref[1], diag, pauli, targets)
    want_rho, want_drho = _reference_rdms(ref, N, N_DIR, SUBSYSTEMS)
    spec, diag_dev = _ket_call(prob, dev)
    expect, dexpect = evolve_tangent(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), tsave, prob["psi0"].to(dev), spec, diag_dev,
                                     d_amp=d_amp.to(dev), d_det=d_det.to(dev), d_u=d_u.to(dev), d_psi0=d_psi.to(dev), flags=_native.TANGENT_RDMS)
    assert tuple(expect.shape) == (N_REAL + 8 + 32, len(tsave), BATCH) and tuple(dexpect.shape) == (N_DIR,) + tuple(expect.shape)
    got_val, got_der = expect[:N_REAL].cpu(), dexpect[:, :N_REAL].cpu()
    val_err = (got_val - want_val).abs().amax(dim=(1, 2)) / _ket_weights(prob)
    print(f"ROW-LAYOUT ket tangent call: values, largest error / row weight {float(val_err.max()):.2e}")
    assert float(val_err.max()) <= VALUE_ATOL  # tests/test_gpu_tangent_matrix.py:53,181
    families = {"diagonal": slice(0, 2), "pauli": slice(2, 4), "overlap": slice(4, 6)}
    for d in range(N_DIR):
        scale, err = float(want_der[d].abs().max()), float((got_der[d] - want_der[d]).abs().max())
        print(f"ROW-LAYOUT ket tangent call: direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
        assert all(float(want_der[d, sl].abs().max()) > 1e-2 for sl in families.values())  # tests/test_gpu_tangent_matrix.py:177
        assert err <= ORACLE_RTOL * scale  # tests/test_gpu_tangent_matrix.py:178
    got_rho, got_drho = _native_rdms(expect[N_REAL:], dexpect[:, N_REAL:], spec.rdms)
    dpsi_norm = ref[1].norm(dim=2).amax(dim=(0, 2))
    for o, qs in enumerate(SUBSYSTEMS):
        assert float((got_rho[o] - want_rho[o]).abs().max()) <= VALUE_ATOL  # tests/test_gpu_rdm_tangent.py:136
        for d in range(N_DIR):
            scale, err = float(want_drho[o][d].abs().max()), float((got_drho[o][d] - want_drho[o][d]).abs().max())
            print(f"ROW-LAYOUT ket tangent call: A={qs} direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
            assert scale > 1e-3 * float(dpsi_norm[d])  # tests/test_gpu_rdm_tangent.py:141
            assert err <= ORACLE_RTOL * scale  # tests/test_gpu_rdm_tangent.py:142


# ---- density matrices -------------------------------------------------------------------------------------------------------------
DM_N, DM_NOISE, DM_SAVES = 2, "dephasing", 3
DM_RDM = (1,)
# one row inside each block of the density-matrix rows (diagonal 0-1, Pauli 2-3, fidelity 4-5, purity 6), with a save point
DM_PICKED = {"diagonal": (1, 2), "pauli": (2, 1), "fidelity": (5, 2), "purity": (6, 2)}


def _dm_run(dev, requires_grad):
    case = _oracle_case(DM_N, DM_NOISE)
    ham = _ham_like(case["terms"], dev, requires_grad=requires_grad)
    rdm = ReducedDensityMatrix(DM_RDM)
    res = mesolve(ham, case["psi0"].to(dev), case["tsave"][:DM_SAVES], _noise_model(NOISE[DM_NOISE]), {"tol": 1e-12}, case["obs"] + [rdm],
                  store_states=False)
    return case, ham, rdm, res


def _direction_products(case, ham):
    """<gradient, direction d> for the recorded directions: Re<g_amp, d_amp[d]> + <g_det, d_det[d]> + <g_u, d_u[d]>."""
    g_amp, g_det, g_u = ham.amp_tables.grad.cpu(), ham.det_tables.grad.cpu(), ham.u_pairs.grad.cpu()
    return torch.stack([(g_amp.conj() * case["d_amp"][d]).real.sum() + (g_det * case["d_det"][d]).sum() + (g_u * case["d_u"][d]).sum()
                        for d in range(case["d_amp"].shape[0])])


def test_density_matrix_rows_values_and_one_hot_gradients_of_every_block(cuda_device):
    case, ham, rdm, res = _dm_run(cuda_device, requires_grad=True)
    assert res.states.numel() == 0 and len(res.expect) == 7 and len(res.rdms) == 1
    got = torch.stack(res.expect)
    want_val, want_der = case["val"][:, :DM_SAVES], case["der"][:, :, :DM_SAVES]
    val_err = float((got.detach().cpu() - want_val).abs().max())
    print(f"ROW-LAYOUT dm values: max error {val_err:.2e}")
    assert tuple(got.shape) == (7, DM_SAVES, 1) and val_err < DM_VALUE_ATOL  # tests/test_gpu_dm_tangent.py:52,95
    for block, (row, k) in DM_PICKED.items():
        for t in (ham.amp_tables, ham.det_tables, ham.u_pairs):
            t.grad = None
        got[row, k, 0].backward(retain_graph=True)
        products = _direction_products(case, ham)
        for d in range(products.numel()):
            if d == ZERO_DIRECTION:
                continue
            scale = float(want_der[d].abs().max())  # the direction's largest entry, as in tests/test_gpu_dm_tangent.py:87
            err = abs(float(products[d]) - float(want_der[d, row, k, 0]))
            print(f"ROW-LAYOUT dm gradient of the {block} row, direction {d}: {float(products[d]):+.6e} against {float(want_der[d, row, k, 0]):+.6e}")
            assert scale > 1e-3  # tests/test_gpu_dm_tangent.py:93
            assert err <= TANGENT_RTOL * scale  # tests/test_gpu_dm_tangent.py:53,94
    # the RDM block: the oracle's dense Lindblad solution and autograd through it (tests/test_gpu_dm_rdm.py:245-269)
    terms = case["terms"]
    o = R.HamTerms(DM_N, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                   terms.det_coeff.clone().requires_grad_(True), terms.dt, terms.n_samples, terms.amp_targets, terms.det_targets)
    o.extra_amp = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_amp]
    o.extra_det = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_det]
    psi0 = case["psi0"][:, 0]
    o_rho = R.lindblad_magnus_dense(o, R.collapse_operators(DM_N, NOISE[DM_NOISE]), torch.outer(psi0, psi0.conj()), case["tsave"][:DM_SAVES],
                                    h_max=h_max(DM_N))
    o_rdm = reduced_density_matrix(rdm, o_rho[..., None])
    assert tuple(res.rdms[0].shape) == tuple(o_rdm.shape) == (DM_SAVES, 1, 2, 2)
    assert float((res.rdms[0].detach().cpu() - o_rdm.detach()).abs().max()) < 1e-8  # tests/test_gpu_dm_rdm.py:222,261
    for t in (ham.amp_tables, ham.det_tables, ham.u_pairs):
        t.grad = None
    res.rdms[0][2, 0, 0, 1].imag.backward()  # one row of the RDM block: Im of an off-diagonal entry at the last save point
    o_rdm[2, 0, 0, 1].imag.backward()
    pairs = (("amp", ham.amp_tables.grad[0].cpu(), torch.stack([c.grad for c, _ in o.amp_terms()])),
             ("det", ham.det_tables.grad[0].cpu(), torch.stack([c.grad for c, _ in o.det_terms()])),
             ("u", ham.u_pairs.grad.cpu(), o.u_pairs.grad))
    for name, g, w in pairs:
        scale, err = float(w.abs().max()), float((g - w).abs().max())
        print(f"ROW-LAYOUT dm gradient of the RDM row w.r.t. {name}: largest entry {scale:.3e}, max error {err:.3e}")
        assert scale > 0.0 and err < 1e-7 * scale  # tests/test_gpu_dm_rdm.py:262-269 (rel_err: of the largest entry)


def test_density_matrix_rows_tangents_of_every_block(cuda_device):
    dev = cuda_device
    case = _oracle_case(DM_N, DM_NOISE)
    expect, dexpect = mesolve_tangent(_ham_like(case["terms"], dev), case["psi0"].to(dev), case["tsave"][:DM_SAVES], _noise_model(NOISE[DM_NOISE]),
                                      {"tol": 1e-12}, case["obs"], d_amp=case["d_amp"][:N_DIR].to(dev), d_det=case["d_det"][:N_DIR].to(dev),
                                      d_u=case["d_u"][:N_DIR].to(dev))
    want_val, want_der = case["val"][:, :DM_SAVES], case["der"][:N_DIR, :, :DM_SAVES]
    assert tuple(expect.shape) == tuple(want_val.shape) == (7, DM_SAVES, 1) and tuple(dexpect.shape) == tuple(want_der.shape)
    val_err = float((expect.cpu() - want_val).abs().max())
    print(f"ROW-LAYOUT dm tangent call: values, max error {val_err:.2e}")
    assert val_err < DM_VALUE_ATOL  # tests/test_gpu_dm_tangent.py:52,95
    for d in range(N_DIR):
        scale, err = float(want_der[d].abs().max()), float((dexpect[d].cpu() - want_der[d]).abs().max())
        print(f"ROW-LAYOUT dm tangent call: direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
        assert scale > 1e-3  # tests/test_gpu_dm_tangent.py:93
        assert err <= TANGENT_RTOL * scale  # tests/test_gpu_dm_tangent.py:53,94
