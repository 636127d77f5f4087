"""Tangent sweep of master-equation runs, host side (no GPU): the doubled tangent tables, the row order of mesolve_tangent, the
refusals that need no device, the C ABI's planning of a density-matrix tangent call, and the two reference modules of the GPU tests
(tests/tangent_pair_reference.py, tests/dm_tangent_reference.py with its record tests/golden/dm_tangent_oracle.npz)."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native, lindblad as L, solver as S
from pulser_diff_amd.observables import DensityMatrixObservables, PauliObservable, Purity, ReducedDensityMatrix, StateOverlap
from pulser_diff_amd.shots import ShotRequest
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call
from pulser_diff_amd.utils import DiagonalObservable
from tests.helpers import random_terms, tangent_dense_reference, to_native
from tests.test_dm_observables_host import _dm_call


BOTH = _native.TANGENT_PAIR_TERMS | _native.TANGENT_DENSITY_MATRIX


def _with_pair(p, keep=[]):
    pair_q = np.array([[0, 2]], dtype=np.uint32)
    pair_t = np.zeros((1, 16), dtype=np.complex128)
    keep += [pair_q, pair_t]
    p.n_pair_terms, p.pair_qubits, p.pair_tables = 1, pair_q.ctypes.data, pair_t.ctypes.data


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


def test_doubled_table_tangents_are_the_directional_derivative_of_doubled_tables():
    """doubled_tables is real-linear (the column half conjugates): (f(x + h d) - f(x - h d)) / 2h is f's directional derivative up to
    rounding, for any h.  1e-12 relative to the largest entry: sums and differences of O(1) doubles."""
    n, n_dir = 3, 4
    gen = torch.Generator().manual_seed(31)
    amp, det, u = _randn(gen, 1, 2, 5, cplx=True), _randn(gen, 1, 2, 5), _randn(gen, 3)
    masks = (0b111, 0b010)
    d_amp, d_det, d_u = _randn(gen, n_dir, 1, 2, 5, cplx=True), _randn(gen, n_dir, 1, 2, 5), _randn(gen, n_dir, 3)
    got = L.doubled_table_tangents(d_amp, d_det, d_u, n)
    assert got[0].shape == (n_dir, 1, 4, 5) and got[1].shape == (n_dir, 1, 4, 5) and got[2].shape == (n_dir, 15)
    h = 0.5
    for d in range(n_dir):
        plus = L.doubled_tables(amp + h * d_amp[d], det + h * d_det[d], u + h * d_u[d], masks, masks, n)[:3]
        minus = L.doubled_tables(amp - h * d_amp[d], det - h * d_det[d], u - h * d_u[d], masks, masks, n)[:3]
        for g, a, b in zip(got, plus, minus):
            fd = (a - b) / (2 * h)
            assert float(fd.abs().max()) > 0.1
            assert float((g[d] - fd).abs().max()) <= 1e-12 * float(fd.abs().max())
    # the column half conjugates: a purely imaginary amplitude tangent keeps its sign there
    assert torch.equal(got[0][:, :, 2:], -d_amp.conj())
    assert L.doubled_table_tangents(None, None, None, n) == (None, None, None)


def _ham(n=2):
    from types import SimpleNamespace

    terms = random_terms(n, 5, 0.004, seed=3, local=True)
    amp, det, u, spec = to_native(terms, "cpu", SolverType.DP5_SE)
    return SimpleNamespace(amp_tables=amp, det_tables=det, u_pairs=u, amp_masks=spec.amp_masks, det_masks=spec.det_masks, dt=terms.dt,
                           n_samples=terms.n_samples, _size=n, pair_terms=())


def test_mesolve_tangent_returns_the_rows_in_the_order_of_the_observables(monkeypatch):
    """The native rows are diagonal, Pauli, fidelity, purity; mesolve_tangent hands them back in the caller's order.  evolve_tangent
    is replaced by a recorder that numbers the native rows (no device)."""
    n, n_t, n_dir = 2, 3, 2
    ham = _ham(n)
    seen = {}

    def fake(amp2, det2, u2, tsave, rho0, spec, obs_diag, d_amp=None, d_det=None, d_u=None, d_psi0=None, flags=0):
        seen.update(flags=flags, spec=spec, rho0=rho0, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi0, amp2=amp2)
        rows = spec.dm.rows()
        expect = torch.arange(rows, dtype=torch.float64)[:, None, None].expand(rows, n_t, 1).clone()
        return expect, torch.stack([expect + 100.0 * (d + 1) for d in range(n_dir)])

    monkeypatch.setattr(S, "evolve_tangent", fake)
    target = torch.ones(4, dtype=torch.complex128) / 2
    obs = [Purity(), PauliObservable(n, [(1.0, "XY")]), DiagonalObservable(torch.arange(4, dtype=torch.float64)), StateOverlap(target),
           torch.diag(torch.ones(4, dtype=torch.complex128)), PauliObservable(n, [(0.5, "ZI")])]
    native_row = [5, 2, 0, 4, 1, 3]  # diag 0-1, pauli 2-3, fidelity 4, purity 5
    psi0 = torch.tensor([1.0, 0, 0, 0], dtype=torch.complex128)
    gen = torch.Generator().manual_seed(5)
    d_amp, dpsi = _randn(gen, n_dir, *ham.amp_tables.shape, cplx=True), _randn(gen, n_dir, 4, cplx=True)
    noise = P.SimConfig(noise=("dephasing",), dephasing_rate=0.5).to_noise_model()
    expect, dexpect = L.mesolve_tangent(ham, psi0, torch.linspace(0, 0.008, n_t, dtype=torch.float64), noise, None, obs, d_amp=d_amp, d_psi0=dpsi)
    assert expect.shape == (6, n_t, 1) and dexpect.shape == (n_dir, 6, n_t, 1)
    assert expect[:, 0, 0].tolist() == [float(r) for r in native_row]
    assert dexpect[1, :, 0, 0].tolist() == [200.0 + r for r in native_row]
    spec = seen["spec"]
    assert spec.n_qubits == 2 * n and spec.tol == L.ME_DEFAULT_TOL and not spec.store_states and spec.dm.purity
    assert len(spec.pair_terms) == n and [(a, b) for a, b, _ in spec.pair_terms] == [(0, 2), (1, 3)]  # the dissipator blocks, as in mesolve
    assert seen["d_det"] is None and seen["d_u"] is None and seen["flags"] == BOTH
    assert torch.equal(seen["d_amp"], torch.cat([d_amp, -d_amp.conj()], dim=2)) and seen["d_amp"].shape[2] == seen["amp2"].shape[1]
    # rho0 = |psi><psi|, d rho0 = |dpsi><psi| + |psi><dpsi|, row-major
    want = torch.einsum("dx,y->dxy", dpsi, psi0.conj()) + torch.einsum("x,dy->dxy", psi0, dpsi.conj())
    assert torch.equal(seen["d_psi0"], want.reshape(n_dir, 1, 16)) and seen["rho0"].shape == (1, 16)


def test_refusals_that_need_no_device():
    ham = _ham(2)
    noise = P.SimConfig(noise=("dephasing",), dephasing_rate=0.5).to_noise_model()
    psi0 = torch.tensor([1.0, 0, 0, 0], dtype=torch.complex128)
    ts = torch.linspace(0, 0.008, 3, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="reduced density"):
        L.mesolve_tangent(ham, psi0, ts, noise, None, [Purity(), ReducedDensityMatrix([0])], d_det=torch.ones(1, *ham.det_tables.shape))
    amp2, det2, u2, am2, dm2 = L.doubled_tables(ham.amp_tables, ham.det_tables, ham.u_pairs, ham.amp_masks, ham.det_masks, 2)
    rho0 = torch.zeros(1, 16, dtype=torch.complex128)
    kw = dict(d_det=torch.ones(1, *det2.shape))
    spec = ProblemSpec(4, ham.dt, ham.n_samples, am2, dm2, solver=SolverType.DP5_SE, store_states=False,
                       dm=DensityMatrixObservables(2, purity=True, rdms=[ReducedDensityMatrix([1])]))
    with pytest.raises(NotImplementedError, match="reduced density"):
        S.evolve_tangent(amp2, det2, u2, ts, rho0, spec, **kw)
    kw["flags"] = BOTH
    spec.dm = DensityMatrixObservables(2, purity=True, shots=True)
    with pytest.raises(NotImplementedError, match="shots"):
        S.evolve_tangent(amp2, det2, u2, ts, rho0, spec, **kw)
    spec.dm = DensityMatrixObservables(2, purity=True)
    spec.shots = ShotRequest(3)
    with pytest.raises(NotImplementedError, match="shots"):
        S.evolve_tangent(amp2, det2, u2, ts, rho0, spec, **kw)
    spec.shots = None
    with pytest.raises(NotImplementedError, match="density-matrix"):
        S.evolve_geometry(amp2, det2, u2, ts, rho0, spec, **kw)
    with pytest.raises(NotImplementedError, match="TANGENT_DENSITY_MATRIX"):  # not asked for: refused as it always was
        S.evolve_tangent(amp2, det2, u2, ts, rho0, spec, d_det=kw["d_det"])


def _info():
    info = _native.RydPlanInfo()
    info.spectral_lo, info.spectral_hi, info.flags = -1.0, 1.0, 0
    return info


def test_the_library_plans_a_density_matrix_tangent_call_on_the_host():
    """With RYDIFF_TANGENT_DENSITY_MATRIX the workspace size of a density-matrix problem is non-zero (without the flag it is 0 with
    RYDIFF_ENOTIMPL, as it always was), grows with the directions, and a call that passes every check is stopped by the host-side workspace test; reduced density matrices, shots and
    the geometry sweep stay refused — nothing here touches a device (this test runs without one)."""
    lib = _native.lib()
    call, info = _dm_call(shots=False), _info()
    assert lib.rydiff_tangent_workspace_bytes(ctypes.byref(call.problem), ctypes.byref(info), 1) == 0  # not asked for: as it always was
    assert "RYDIFF_TANGENT_DENSITY_MATRIX" in _native.last_error()
    sizes = [lib.rydiff_tangent_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(info), d, BOTH) for d in (1, 2, 8)]
    state_bytes = 2 * 16 * 16  # B * 4^n * sizeof(complex128)
    assert sizes[0] > 0, _native.last_error()
    assert sizes[1] - sizes[0] >= 2 * state_bytes and sizes[2] - sizes[1] >= 12 * state_bytes

    def forward(mutate=None, geometry=False, flags=BOTH):
        c = _dm_call(shots=False)
        if mutate:
            mutate(c.problem)
        tg = _native.RydTangent()
        tg.n_dir, tg.d_det, tg.flags = 2, 0x1000, flags
        if geometry:
            rc = lib.rydiff_forward_geometry(ctypes.byref(c.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(0x1000), None, None,
                                             ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
        else:
            rc = lib.rydiff_forward_tangent(ctypes.byref(c.problem), ctypes.byref(info), ctypes.byref(tg), ctypes.c_void_p(0x1000), None,
                                            ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), 0, None)
        _native.check(rc)

    with pytest.raises(MemoryError, match="tangent workspace too small"):
        forward()
    with pytest.raises(NotImplementedError, match="n_dm_rdms"):
        forward(lambda p: setattr(p, "n_dm_rdms", 1))
    with pytest.raises(NotImplementedError, match="shots"):
        forward(lambda p: setattr(p, "n_shots", 4))
    with pytest.raises(NotImplementedError, match="shard"):
        forward(lambda p: setattr(p, "shard_bits", 1))
    with pytest.raises(NotImplementedError, match="conditioned"):
        forward(lambda p: setattr(p, "amp_conditioned_terms", 1))
    with pytest.raises(NotImplementedError, match="dm_atoms"):
        forward(geometry=True)
    with pytest.raises(NotImplementedError, match="RYDIFF_TANGENT_DENSITY_MATRIX"):
        forward(flags=0)
    with pytest.raises(NotImplementedError, match="RYDIFF_TANGENT_PAIR_TERMS"):  # (a pair term without its flag)
        forward(_with_pair, flags=_native.TANGENT_DENSITY_MATRIX)
    with pytest.raises(ValueError, match="flags"):
        forward(flags=BOTH | 8)
    assert lib.rydiff_geometry_workspace_bytes_flags(ctypes.byref(call.problem), ctypes.byref(info), 2, BOTH) == 0
    assert "dm_atoms" in _native.last_error()


def test_run_sensitivities_route_argument():
    from tests.test_tangent_host import _basic_usage_emulator, _params

    prm = _params()
    emu = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"])
    obs = DiagonalObservable(torch.ones(16, dtype=torch.float64))
    with pytest.raises(ValueError, match="route"):
        emu.run_sensitivities([prm["omega"]], [obs], route="loop")
    with pytest.raises(TypeError, match="master-equation"):  # a ket has no Purity / fidelity row on this path
        emu.run_sensitivities([prm["omega"]], [Purity()])
    noisy = _basic_usage_emulator(prm["q0"], prm["omega"], prm["area"], prm["phase"], config=P.SimConfig(noise="dephasing"))
    with pytest.raises(NotImplementedError, match="ReducedDensityMatrix"):
        noisy.run_sensitivities([prm["omega"]], [ReducedDensityMatrix([0])])


def test_pair_reference_without_blocks_is_the_helper_and_both_exponential_routes_agree():
    """tests.tangent_pair_reference: with no pair term it is tests.helpers.tangent_dense_reference (1e-13: the same exponentials);
    with blocks, the dense block exponential and the action on vectors agree at 1e-12 relative (both exact to rounding)."""
    from tests.tangent_pair_reference import embed_pair, tangent_pair_reference

    n, n_dir, batch = 4, 3, 2
    terms = random_terms(n, 21, 0.005, seed=61, local=True, phase=True)
    gen = torch.Generator().manual_seed(77)
    ka, kd = len(terms.amp_terms()), len(terms.det_terms())
    d_amp, d_det, d_u = _randn(gen, n_dir, ka, 21, cplx=True), _randn(gen, n_dir, kd, 21), _randn(gen, n_dir, 6)
    psi0 = _randn(gen, 16, batch, cplx=True)
    d_psi = _randn(gen, n_dir, 16, batch, cplx=True)
    tsave = torch.tensor([0.0, 0.022, 0.048], dtype=torch.float64)
    for solver in (SolverType.KRYLOV_SE, SolverType.DP5_SE):
        want = tangent_dense_reference(terms, d_amp, d_det, d_u, psi0, d_psi, tsave, solver)
        for dense in (True, False):
            got = tangent_pair_reference(terms, (), d_amp, d_det, d_u, psi0, d_psi, tsave, solver, dense=dense)
            for g, w in zip(got, want):
                assert float((g - w).abs().max()) <= 1e-13 * float(w.abs().max())
        pairs = tuple((int(a), int(b), 0.7 * _randn(gen, 4, 4, cplx=True).numpy()) for a, b in ((0, 3), (2, 1), (3, 1)))
        a = tangent_pair_reference(terms, pairs, d_amp, d_det, d_u, psi0, d_psi, tsave, solver, dense=True)
        b = tangent_pair_reference(terms, pairs, d_amp, d_det, d_u, psi0, d_psi, tsave, solver, dense=False)
        for x, y in zip(a, b):
            assert float((x - y).abs().max()) <= 1e-12 * float(x.abs().max())
        assert float((a[1] - want[1]).abs().max()) > 1e-3  # the blocks do act
    # the embedding: qubit q is bit n - 1 - q, block index 2 * bit_a + bit_b — against kron on neighbouring qubits
    blk = _randn(gen, 4, 4, cplx=True)
    want = torch.kron(torch.kron(torch.eye(2, dtype=torch.complex128), blk), torch.eye(2, dtype=torch.complex128))
    assert torch.equal(embed_pair(4, 1, 2, blk.numpy()), want)


def test_the_recorded_oracle_is_what_the_generator_computes():
    """The smallest recorded case against a fresh computation: the inputs bit for bit (seeded), the values at 1e-13 and a seeded
    contraction w . J of the Jacobian — one reverse pass instead of the 28 of the full Jacobian — at 1e-10 relative."""
    from oracle import restatement as R
    from tests import dm_tangent_reference as D
    from tests.helpers import shifted_terms
    from tests.test_gpu_dm_observables import _torch_rows

    n, noise_key = 2, "dephasing"
    rec = D.load_case(n, noise_key)
    inp = D.case_inputs(n, noise_key)
    for k, v in inp.items():
        assert torch.equal(rec[k], v), k
    assert rec["val"].shape == (7, 4, 1) and rec["der"].shape == (D.N_DIR, 7, 4, 1)
    assert float(rec["der"][D.ZERO_DIRECTION].abs().max()) == 0.0
    terms, obs = D.case_terms(n), D.observables(n, inp["target"])
    s = torch.zeros(D.N_DIR, dtype=torch.float64, requires_grad=True)
    rho = R.lindblad_magnus_dense(shifted_terms(terms, inp["d_amp"][:, 0], inp["d_det"][:, 0], inp["d_u"], s), R.collapse_operators(n, D.NOISE[noise_key]),
                                  torch.outer(inp["psi0"][:, 0], inp["psi0"][:, 0].conj()), torch.tensor(D.TSAVE, dtype=torch.float64), h_max=D.h_max(n))
    rows = torch.stack(_torch_rows(rho[..., None], obs))
    assert float((rows.detach() - rec["val"]).abs().max()) <= 1e-13
    w = _randn(torch.Generator().manual_seed(9), *rows.shape)
    (g,) = torch.autograd.grad((w * rows).sum(), s)
    want = (w[None] * rec["der"]).sum(dim=(1, 2, 3))
    assert float(want.abs().max()) > 1e-2
    assert float((g - want).abs().max()) <= 1e-10 * float(want.abs().max())
    for nn in D.SIZES:  # every case of the GPU test is in the record
        for nk in D.NOISE:
            assert D.load_case(nn, nk)["der"].shape == (D.N_DIR, 7, 4, D.BATCH[nn])
