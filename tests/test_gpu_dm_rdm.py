"""Reduced density matrices of master-equation runs (RydProblem.n_dm_rdms / dm_rdm_masks; k_dm_rdm / k_dm_rdm_scatter in
csrc/dm_kernels.hpp): partial traces of rho evaluated while it is on the device and differentiated through the grad_states route.

Kernel families (asserted from the plan): 2 / 3 atoms on the one-wave lane sweep, 4 atoms on the one-workgroup persistent sweep, 7 atoms
on the direct kernels, 9 atoms (B = 2) on the chained tile passes.  9 atoms is the smallest size at which a thread of k_dm_rdm sums more
than one e at m = 1 (2^8 settings of E on 2^7 slices) and k_dm_rdm_scatter runs more than one block of y per row index a.

References and bars:
  values      tests/dm_rdm_reference.py (reshape to 2n axes, einsum over the traced ones) on the very vectors the call stored, random
              complex and non-Hermitian as matrices: |got - want| <= 1e-12 * sum|terms| per entry.  An entry is a fixed-order sum of at
              most 2^(n-m) <= 2^9 terms here, worst-case rounding N * 2^-53 * sum|terms| < 2.3e-13 * sum|terms| even at the library's
              limit of 2^11 terms.  Two identical calls return bitwise equal rows (one owner per output, no atomics).
  cotangent   the dense matrix rydiff.h writes down, entry by entry: 64 * 2^-52 * sum|contributions to the entry| (COT_BAR of
              tests/test_gpu_dm_observables_wide.py)
  end to end  the oracle's dense Lindblad solution at 1e-8; gradients against the stored-rho torch route of the same build at 1e-10 and
              against the oracle's differentiable dense Magnus integrator at 1e-7 (tsave 1e-6) — the bars tests/test_gpu_dm_observables.py
              uses for the other row kinds, with its noise settings and save times."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd import pulses as pl
from pulser_diff_amd import solver as S
from pulser_diff_amd.lindblad import mesolve
from pulser_diff_amd.observables import DensityMatrixObservables, ReducedDensityMatrix, reduced_density_matrix
from pulser_diff_amd.solver import SolverType, evolve, split_observables
from tests.dm_rdm_reference import partial_trace, rdm_cotangent_reference, rdm_rows_reference
from tests.helpers import dm_cotangent_reference, dm_rows_reference, random_terms, rel_err, to_native
from tests.test_gpu_dm_observables import ME_BATCH, ME_NOISE, ME_TSAVE, _me_reference, _paulis
from tests.test_gpu_dm_observables_wide import CHAINED, COT_BAR, DIRECT, LANES, PERSISTENT, TSAVE, _flip_paulis, _problem, _randn, _route_inputs
from tests.test_gpu_master_equation_sizes import NON_NORMAL, _ham_like, _noise_model, _random_kets
from tests.test_gpu_workspace_contents import _filled

pytestmark = pytest.mark.gpu

FAMILY = {2: LANES, 3: LANES, 4: PERSISTENT, 7: DIRECT, 9: CHAINED}
VALUE_RTOL = 1e-12
ROUTE_RTOL = 1e-10


def _mask(*atoms):
    return sum(1 << a for a in atoms)


# per size, in this order: a single atom; the trailing atom in A; the trailing atom not in A; non-adjacent atoms; the widest (m = n at
# two atoms, m = 6 at 7 and 9); then mixed m up to eight matrices (masks may share atoms)
MASKS = {
    2: [_mask(0), _mask(1), _mask(0), _mask(0, 1), _mask(1, 0), _mask(1), _mask(0, 1), _mask(0)],
    4: [_mask(1), _mask(1, 3), _mask(0, 2), _mask(0, 3), _mask(0, 1, 2, 3), _mask(2), _mask(1, 2, 3), _mask(0, 1)],
    7: [_mask(3), _mask(6), _mask(0, 2, 5), _mask(1, 4, 6), _mask(0, 1, 2, 3, 4, 6), _mask(0, 1, 2, 3, 4, 5), _mask(2, 3), _mask(0, 5, 6)],
    9: [_mask(0), _mask(8), _mask(1, 4, 7), _mask(0, 3, 8), _mask(0, 2, 3, 5, 6, 8), _mask(1, 2, 3, 4, 5, 6), _mask(4), _mask(7, 8)],
}


def _rdm_rows(masks):
    return sum(2 * 4 ** bin(m).count("1") for m in masks)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the definitions
# ----------------------------------------------------------------------------------------------------------------------
def _values_call(dev, n, masks, with_others, v0, diag, targets):
    amp, det, u, spec = _problem(n, dev)
    if with_others:
        spec.dm = DensityMatrixObservables(n, diag=diag.to(dev), pauli=_paulis(n), targets=targets.to(dev), purity=True, rdms=list(masks))
    else:
        spec.dm = DensityMatrixObservables(n, rdms=list(masks))
    states, expect = evolve(amp, det, u, torch.tensor(TSAVE, dtype=torch.float64), v0.to(dev), spec, None)
    torch.cuda.synchronize()
    assert spec.options["_last_stats"]["kernel_family"] == FAMILY[n], spec.options["_last_stats"]
    return states.cpu().numpy(), expect.cpu().numpy()


@pytest.mark.parametrize("n", [2, 4, 7, 9])
def test_every_entry_matches_the_dense_partial_trace(cuda_device, n):
    """Eight RDMs of mixed m next to two diagonal rows, two Pauli observables, three fidelities and the purity (the row offsets), then
    the first five alone (RDM rows as the only density-matrix request); random complex non-Hermitian vectors, B = 2, three save
    points, states stored so that the reference works on the very vectors the call returned."""
    dim, batch = 2 ** n, 2
    gen = torch.Generator().manual_seed(9100 + n)
    v0 = _randn(gen, batch, dim * dim, cplx=True)
    diag = _randn(gen, 2, dim)
    targets = _randn(gen, 3, 1, dim, cplx=True)
    for tag, masks, with_others in (("with-all-row-kinds", MASKS[n], True), ("alone", MASKS[n][:5], False)):
        st, got = _values_call(cuda_device, n, masks, with_others, v0, diag, targets)
        n_other = 2 + 2 + 3 + 1 if with_others else 0
        assert got.shape == (n_other + _rdm_rows(masks), len(TSAVE), batch)
        assert np.array_equal(st[0], v0.numpy())
        worst = 0.0
        for k in range(len(TSAVE)):
            for b in range(batch):
                want, tot = rdm_rows_reference(st[k, b], n, masks)
                if with_others:
                    w2, t2 = dm_rows_reference(st[k, b], n, diag.numpy(), _paulis(n), targets[:, 0].numpy(), True)
                    want, tot = np.concatenate([w2, want]), np.concatenate([t2, tot])
                ratio = np.abs(got[:, k, b] - want) / tot
                worst = max(worst, float(ratio[n_other:].max()))
                assert (ratio <= VALUE_RTOL).all(), (tag, k, b, np.flatnonzero(ratio > VALUE_RTOL)[:8], ratio.max())
        print(f"DM-RDM-VAL n={n} {tag}: {worst:.2e} of sum|terms| (bar {VALUE_RTOL:.0e})")
        # no Hermiticity is assumed: entry (a, a') and its transpose are computed independently and differ from conjugates here
        d = 2 ** bin(masks[3]).count("1")
        block = got[n_other + _rdm_rows(masks[:3]):][:2 * d * d]  # (the rows of RDM 3 start behind those of RDMs 0..2)
        rho_a = (block[0::2] + 1j * block[1::2]).reshape(d, d, len(TSAVE), batch)
        assert np.abs(rho_a[0, 1] - rho_a[1, 0].conj()).min() > 1e-3
        st2, again = _values_call(cuda_device, n, masks, with_others, v0, diag, targets)
        assert np.array_equal(got[n_other:, 0], again[n_other:, 0])  # bitwise: one owner per output, a fixed order of the slices
        if np.array_equal(st, st2):
            assert np.array_equal(got[n_other:], again[n_other:])


def test_split_observables_returns_the_matrices_in_the_order_of_the_qubits(cuda_device):
    """ReducedDensityMatrix objects with non-ascending qubits: the rows come back permuted by native_index into the user's order."""
    n, batch = 4, 2
    dim = 2 ** n
    gen = torch.Generator().manual_seed(9300)
    v0 = _randn(gen, batch, dim * dim, cplx=True)
    obs = [ReducedDensityMatrix([3, 0]), ReducedDensityMatrix([2]), ReducedDensityMatrix([1, 3, 0])]
    amp, det, u, spec = _problem(n, cuda_device)
    spec.dm = DensityMatrixObservables(n, purity=True, rdms=obs)
    states, expect = evolve(amp, det, u, torch.tensor(TSAVE, dtype=torch.float64), v0.to(cuda_device), spec, None)
    real, ov, rdms = split_observables(expect, 0, obs)
    assert real.shape[0] == 1 and ov is None and len(rdms) == 3
    st = states.cpu().numpy()
    for o, got in zip(obs, rdms):
        assert got.shape == (len(TSAVE), batch, 2 ** o.n_sub, 2 ** o.n_sub)
        for k in range(len(TSAVE)):
            for b in range(batch):
                want = partial_trace(st[k, b].reshape(dim, dim), n, o.qubits)
                tot = partial_trace(np.abs(st[k, b]).reshape(dim, dim), n, o.qubits)
                assert (np.abs(got[k, b].cpu().numpy() - want) <= VALUE_RTOL * tot).all(), (o.qubits, k, b)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the cotangent, entry by entry
# ----------------------------------------------------------------------------------------------------------------------
# composition -> (RDM masks by size, diagonal tables, Pauli rows, fidelities, purity)
COT_MASKS = {4: {"alone": [_mask(1), _mask(0, 3)], "overlapping": [_mask(0, 1, 3), _mask(1, 2), _mask(1)],
                 "all": [_mask(3), _mask(0, 2), _mask(0, 1, 2, 3)]},
             9: {"alone": [_mask(4), _mask(0, 8)], "overlapping": [_mask(1, 4, 8), _mask(4, 5), _mask(8)],
                 "all": [_mask(8), _mask(0, 3, 7), _mask(0, 2, 3, 5, 6, 8)]}}
COMPOSITIONS = {
    "a-rdm-rows-alone": ("alone", 0, None, 0, False),
    "b-two-and-three-overlapping-masks": ("overlapping", 0, None, 0, False),
    "c-rdms-with-diag-and-flip-strings": ("overlapping", 2, _flip_paulis, 0, False),
    "d-everything": ("all", 2, _paulis, 3, True),
}


@pytest.mark.parametrize("comp", list(COMPOSITIONS))
@pytest.mark.parametrize("n", [4, 9])
def test_cotangent_entry_by_entry(cuda_device, n, comp):
    """Only save point 0 (= psi0) carries weight, so psi0.grad IS the cotangent launch_observable_cotangent formed there.  Some weights
    are exact zeros: whole entries (gRe = gIm = 0: the skip in k_dm_rdm_scatter), single parts, and one whole row of another kind."""
    which, n_diag, make_paulis, n_fid, purity = COMPOSITIONS[comp]
    masks = COT_MASKS[n][which]
    dim, batch = 2 ** n, 2
    gen = torch.Generator().manual_seed(9400 + n)
    amp, det, u, spec = _problem(n, cuda_device)
    v0 = _randn(gen, batch, dim * dim, cplx=True)
    diag = _randn(gen, max(n_diag, 1), dim)[:n_diag]
    targets = _randn(gen, max(n_fid, 1), 1, dim, cplx=True)[:n_fid]
    paulis = make_paulis(n) if make_paulis else []
    spec.dm = DensityMatrixObservables(n, diag=diag.to(cuda_device) if n_diag else None, pauli=paulis or None,
                                       targets=targets.to(cuda_device) if n_fid else None, purity=purity, rdms=masks)
    n_rows, n_rdm = spec.dm.rows(), _rdm_rows(masks)
    n_other = n_rows - n_rdm
    w = torch.zeros(n_rows, len(TSAVE), batch, dtype=torch.float64)
    w[:, 0] = _randn(gen, n_rows, batch)
    w[n_other + 2:n_other + 4, 0, :] = 0.0  # entry (0, 1) of the first RDM, Re and Im, both trajectories
    w[n_other + 5, 0, 0] = 0.0              # Im of entry (0, 2) (or (1, 0) at m = 1), trajectory 0
    w[n_rows - 2, 0, 1] = 0.0               # Re of the last entry of the last RDM, trajectory 1
    if n_other:
        w[0, 0, :] = 0.0
    psi0 = v0.to(cuda_device).requires_grad_(True)
    _, expect = evolve(amp, det, u, torch.tensor(TSAVE, dtype=torch.float64), psi0, spec, None)
    assert spec.options["_last_stats"]["kernel_family"] == FAMILY[n], spec.options["_last_stats"]
    assert expect.shape == w.shape
    (expect * w.to(cuda_device)).sum().backward()
    torch.cuda.synchronize()
    got = psi0.grad.cpu().numpy()
    assert np.isfinite(got).all(), (comp, np.argwhere(~np.isfinite(got))[:8])
    worst = 0.0
    for b in range(batch):
        g = w[:, 0, b].numpy()
        want, tot = rdm_cotangent_reference(n, masks, g[n_other:])
        if n_other:
            c, t = dm_cotangent_reference(v0[b].numpy(), n, g[:n_other], diag.numpy(), paulis, targets[:, 0].numpy() if n_fid else (), purity)
            want, tot = want + c, tot + t
        err = np.abs(got[b] - want)
        bad = np.flatnonzero(~(err <= COT_BAR * tot))
        assert bad.size == 0, (comp, b, bad[:8] // dim, bad[:8] % dim, err[bad[:8]], tot[bad[:8]])
        assert (tot > 0).any()
        worst = max(worst, float((err[tot > 0] / tot[tot > 0]).max()))
    print(f"DM-RDM-COT n={n} {comp}: {worst:.2e} of sum|contributions| (bar {COT_BAR:.2e})")


# ----------------------------------------------------------------------------------------------------------------------
# 3. end to end, without stored states
# ----------------------------------------------------------------------------------------------------------------------
ME_RDMS = {3: ([0, 1], [2], [2, 0]), 4: ([1, 3], [0], [3, 2, 0])}


@pytest.mark.parametrize("n", [3, 4])
def test_native_rdms_match_the_dense_lindblad_solution_without_stored_states(cuda_device, n):
    terms, psi0, ref = _me_reference(n)
    obs = [ReducedDensityMatrix(q) for q in ME_RDMS[n]]
    res = mesolve(_ham_like(terms, cuda_device), psi0.to(cuda_device), torch.tensor(ME_TSAVE[n], dtype=torch.float64), _noise_model(ME_NOISE[n]),
                  observables=obs, store_states=False)
    assert res.stats["kernel_family"] == FAMILY[n], res.stats
    assert res.states.numel() == 0 and res.expect == [] and len(res.rdms) == len(obs)
    for o, got in zip(obs, res.rdms):
        assert got.shape == (len(ME_TSAVE[n]), ME_BATCH[n], 2 ** o.n_sub, 2 ** o.n_sub) and got.is_complex()
        want = np.stack([np.stack([partial_trace(ref[k, :, :, b].numpy(), n, o.qubits) for b in range(ME_BATCH[n])])
                         for k in range(len(ME_TSAVE[n]))])
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f"DM-RDM-ME n={n} qubits={o.qubits}: {err:.2e}")
        assert err < 1e-8, o.qubits


def _functional(rdms, weights):
    """sum |rho_A|^2 plus a linear functional with fixed random complex weights, over all RDMs and save points."""
    return sum((r.real ** 2 + r.imag ** 2).sum() + (r * w.to(r.device)).sum().real for r, w in zip(rdms, weights))


def _weights(n, n_t, batch, seed):
    gen = torch.Generator().manual_seed(seed)
    return [_randn(gen, n_t, batch, 2 ** len(q), 2 ** len(q), cplx=True) for q in ME_RDMS[n]]


@pytest.mark.parametrize("n", [3, 4])
def test_gradients_match_dense_autograd(cuda_device, n):
    """Non-normal noise, every save point weighted: amp, det, u_pairs and tsave against autograd through the oracle's dense Magnus
    integrator."""
    terms = random_terms(n, 8, 0.004, seed=810 + n, local=True)
    noise = {"depolarizing": 0.8, "eff_noise": [(0.6, NON_NORMAL)]}
    tsave0 = torch.tensor([0.0, 0.0067, 0.0158, 0.0243], dtype=torch.float64)
    psi0 = _random_kets(2 ** n, 1, seed=820 + n)
    obs = [ReducedDensityMatrix(q) for q in ME_RDMS[n]]
    weights = _weights(n, 4, 1, 9500 + n)
    o = R.HamTerms(n, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                   terms.det_coeff.clone().requires_grad_(True), terms.dt, terms.n_samples, terms.amp_targets, terms.det_targets)
    o.extra_amp = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_amp]
    o.extra_det = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_det]
    o_ts = tsave0.clone().requires_grad_(True)
    o_rho = R.lindblad_magnus_dense(o, R.collapse_operators(n, noise), torch.outer(psi0[:, 0], psi0[:, 0].conj()), o_ts,
                                    h_max=0.0002 if n < 4 else 0.0004)
    o_rdms = [reduced_density_matrix(ob, o_rho[..., None]) for ob in obs]
    _functional(o_rdms, weights).backward()

    ham = _ham_like(terms, cuda_device, requires_grad=True)
    ts = tsave0.clone().requires_grad_(True)
    res = mesolve(ham, psi0.to(cuda_device), ts, _noise_model(noise), options={"tol": 1e-12}, observables=obs, store_states=False)
    assert res.stats["kernel_family"] == FAMILY[n] and res.states.numel() == 0, res.stats
    _functional(res.rdms, weights).backward()
    for ob, g, w in zip(obs, res.rdms, o_rdms):
        assert float((g.detach().cpu() - w.detach()).abs().max()) < 1e-8, ob.qubits
    pairs = (("amp", ham.amp_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c, _ in o.amp_terms()]).numpy(), 1e-7),
             ("det", ham.det_tables.grad[0].cpu().numpy(), torch.stack([c.grad for c, _ in o.det_terms()]).numpy(), 1e-7),
             ("u", ham.u_pairs.grad.cpu().numpy(), o.u_pairs.grad.numpy(), 1e-7),
             ("tsave", ts.grad.numpy(), o_ts.grad.numpy(), 1e-6))
    for name, got, want, bar in pairs:
        err = rel_err(got, want)
        print(f"DM-RDM-GRAD n={n} {name}: {err:.2e}")
        assert err < bar, name


def _me_route(n, dev, native, batch=2, seed=960):
    """The functional and its gradients through the native RDM rows (no stored states) or through stored rho and the torch route."""
    terms = random_terms(n, 12, 0.004, seed=seed + n, local=True)
    noise = {"depolarizing": 0.9, "eff_noise": [(0.5, NON_NORMAL)]}
    psi0 = _random_kets(2 ** n, batch, seed=seed + 10 + n)
    obs = [ReducedDensityMatrix(q) for q in ME_RDMS[n]]
    weights = _weights(n, 4, batch, seed + 20 + n)
    ham = _ham_like(terms, dev, requires_grad=True)
    ts = torch.tensor([0.0, 0.0093, 0.027, 0.041], dtype=torch.float64, requires_grad=True)
    if native:
        res = mesolve(ham, psi0.to(dev), ts, _noise_model(noise), observables=obs, store_states=False)
        assert res.states.numel() == 0
        rdms = res.rdms
    else:
        res = mesolve(ham, psi0.to(dev), ts, _noise_model(noise))
        rdms = [reduced_density_matrix(o, res.states) for o in obs]
    assert res.stats["kernel_family"] == FAMILY[n], res.stats
    _functional(rdms, weights).backward()
    torch.cuda.synchronize()
    out = {f"rdm{i}": torch.view_as_real(r.detach()).cpu().numpy() for i, r in enumerate(rdms)}
    out.update({"amp": ham.amp_tables.grad.cpu().numpy(), "det": ham.det_tables.grad.cpu().numpy(), "u": ham.u_pairs.grad.cpu().numpy(),
                "tsave": ts.grad.numpy()})
    return out


@pytest.mark.parametrize("n", [3, 4])
def test_gradients_agree_with_the_stored_rho_route(cuda_device, n):
    got, want = _me_route(n, cuda_device, True), _me_route(n, cuda_device, False)
    for key in want:
        err = rel_err(got[key], want[key])
        print(f"DM-RDM-ROUTES n={n} {key}: {err:.2e}")
        assert err < ROUTE_RTOL, key


# ----------------------------------------------------------------------------------------------------------------------
# 4. workspace
# ----------------------------------------------------------------------------------------------------------------------
def _nine_atom_run(dev):
    """18 doubled qubits, B = 1, RDM rows as the only density-matrix request, no stored states, gradients on every leaf."""
    terms, psi, _, _, _ = _route_inputs(18)
    masks = MASKS[9][:4] + [_mask(2, 3, 5)]
    amp, det, u, spec = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=False)
    spec.tape = "full"
    spec.dm = DensityMatrixObservables(9, rdms=masks)
    leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True),
              torch.tensor((0.0, 0.0041, 0.0102, 0.0163), dtype=torch.float64, requires_grad=True), psi.to(dev).requires_grad_(True)]
    _, expect = evolve(*leaves, spec, None)
    assert spec.options["_last_stats"]["kernel_family"] == DIRECT, spec.options["_last_stats"]
    w = _randn(torch.Generator().manual_seed(9600), *expect.shape).to(dev)
    grads = torch.autograd.grad((w * expect).sum(), leaves)
    torch.cuda.synchronize()
    return [expect.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads]


def test_a_poisoned_workspace_changes_nothing(cuda_device, monkeypatch):
    """Every workspace filled with quiet NaNs against zero-filled ones: the scratch trajectory the rows are evaluated from and the
    cotangent buffer (cleared by the dense pass of launch_dm_apply where only RDM rows write it) are written before they are read."""
    out = {}
    for name, value in (("zeros", 0.0), ("nans", float("nan"))):
        monkeypatch.setattr(S, "_new_workspace", _filled(value))
        out[name] = _nine_atom_run(cuda_device)
    for label, a, b in zip(("rows", "amp", "det", "u", "tsave", "psi0"), out["nans"], out["zeros"]):
        assert np.isfinite(a).all(), f"{label}: a region is read before it is written"
        assert rel_err(a, b) < 1e-12, label


def _device_call(dev, masks, purity):
    """A _Call on the doubled register of two atoms whose tables live on the device (rydiff_plan reads them)."""
    nq = 4
    dm = DensityMatrixObservables(2, purity=purity, rdms=list(masks) or None)
    spec = S.ProblemSpec(nq, 0.004, 5, (2 ** nq - 1,), (2 ** nq - 1,), solver=SolverType.DP5_SE, dm=dm)
    return S._Call(spec, torch.zeros(1, 1, 5, dtype=torch.complex128, device=dev), torch.zeros(1, 1, 5, dtype=torch.float64, device=dev),
                   torch.zeros(nq * (nq - 1) // 2, dtype=torch.float64, device=dev), np.linspace(0, 0.008, 3), 2, None)


def test_the_plan_counts_rdm_rows_as_a_live_request(cuda_device):
    """rydiff_plan's workspace: n_dm_rdms = 0 changes nothing; RDM rows alone get the trajectory the one-launch sweeps are evaluated
    from, exactly as the purity alone does; dm_atoms = 0 ignores the fields."""
    def planned(call, need_tape=1, backward=1):
        scratch = torch.zeros(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=cuda_device)
        info = _native.RydPlanInfo()
        _native.check(_native.lib().rydiff_plan(ctypes.byref(call.problem), need_tape, backward, ctypes.c_void_p(scratch.data_ptr()), None,
                                                ctypes.byref(info)))
        torch.cuda.synchronize()
        return int(info.workspace_bytes)

    nothing, purity_only = planned(_device_call(cuda_device, (), False)), planned(_device_call(cuda_device, (), True))
    assert purity_only > nothing
    assert planned(_device_call(cuda_device, (0b11, 0b01), False)) == purity_only
    assert planned(_device_call(cuda_device, (0b11, 0b01), True)) == purity_only
    unused = _device_call(cuda_device, (0b11,), False)
    unused.problem.n_dm_rdms = 0
    assert planned(unused) == nothing
    off, plain = _device_call(cuda_device, (0b11,), False), _device_call(cuda_device, (), False)
    off.problem.dm_atoms = plain.problem.dm_atoms = 0
    off.problem.n_qubits = plain.problem.n_qubits = 4
    assert planned(off) == planned(plain)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the emulator
# ----------------------------------------------------------------------------------------------------------------------
def _emulator(n=3):
    seq = pl.Sequence(pl.Register.rectangle(1, n, spacing=8, prefix="q"), pl.MockDevice)
    seq.declare_channel("g", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(300, 2.4), pl.RampWaveform(300, -3.0, 2.0), 0.2), "g")
    cfg = P.SimConfig(noise=("dephasing",), dephasing_rate=1.0)
    return P.TorchEmulator.from_sequence(seq, config=cfg, evaluation_times=[0.05 * k for k in range(1, 7)])


def test_emulator_serves_native_rdms_without_stored_states(cuda_device):
    pair, single = ReducedDensityMatrix([0, 1]), ReducedDensityMatrix([2])
    res = _emulator().run(observables=[pair, single], store_states=False)
    assert res._states_tbd.numel() == 0
    stored = _emulator().run()  # the stored-rho route: the torch partial trace of results.reduced_density_matrix
    assert stored.states.ndim == 4
    for name, obs in (("pair", pair), ("single", single)):
        a, b = res.reduced_density_matrix(obs), stored.reduced_density_matrix(obs)
        assert a.shape == b.shape == (len(res), 1, 2 ** obs.n_sub, 2 ** obs.n_sub)
        err = float((a - b).abs().max())
        print(f"DM-RDM-EMU {name}: {err:.2e}")
        assert err < ROUTE_RTOL, name
        trace = torch.einsum("tbaa->tb", a)
        assert float((trace - 1.0).abs().max()) < 1e-8, name
    assert res.reduced_density_matrix(pair) is res._native_rdms[0] and res.reduced_density_matrix(single) is res._native_rdms[1]
    entropy = res.entanglement_entropy(single)
    assert entropy.shape == (len(res), 1) and float(entropy[-1, 0]) > float(entropy[0, 0]) >= 0.0  # the single-atom entropy grows (from the product state at t = 0)
    neg = res.negativity(pair, 1)
    assert neg.shape == (len(res), 1) and bool(torch.isfinite(neg).all()) and bool((neg >= 0).all())
    assert float((neg - stored.negativity(pair, 1)).abs().max()) < 1e-8


def test_refusals(cuda_device, monkeypatch):
    from tests.test_host_logic import _three_level_emulator

    def no_launch(*a, **k):
        raise AssertionError("the solver was launched")

    import pulser_diff_amd.lindblad as L

    sim = _emulator()
    monkeypatch.setattr(L, "evolve", no_launch)
    with pytest.raises(NotImplementedError, match="store_states=False") as info:  # stored states: refused before any launch
        sim.run(observables=[ReducedDensityMatrix([0, 1])])
    assert "ReducedDensityMatrix" in str(info.value) and "master-equation" in str(info.value)
    assert "results.reduced_density_matrix(obs)" in str(info.value)
    with pytest.raises(ValueError, match="outside"):
        sim.run(observables=[ReducedDensityMatrix([3])], store_states=False)
    monkeypatch.undo()
    three, _ = _three_level_emulator(compute_device="cuda", n=2)
    with pytest.raises(NotImplementedError, match="three-level"):
        three.run(solver=SolverType.KRYLOV_SE, observables=[ReducedDensityMatrix((0,))], store_states=False)
