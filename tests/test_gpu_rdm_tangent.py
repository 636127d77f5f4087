"""Reduced-density-matrix tangents from the tangent sweep (k_rdm_tangent<M>, RYDIFF_TANGENT_RDMS):
d rho_A = Tr_E(|dpsi_d><psi| + |psi><dpsi_d|) at every evaluation time, every direction.

1. Entry by entry against the dense forward-mode reference (tests.helpers.tangent_dense_reference; d rho formed here by a reshape
   and an einsum of its states and tangent states): values at VALUE_ATOL = 1e-9 absolute (tests/test_gpu_rdm_observables.py),
   tangents at ORACLE_RTOL = 1e-8 of the direction's largest entry (tests/test_gpu_tangent.py); the largest |d rho| entry of every
   direction and RDM must exceed 1e-3 of the largest ||dpsi_d|| (nothing passes on zeros).  1 qubit (no environment, row stride 2),
   3 qubits (m = 1, 2, 3), 6 qubits (m = 4, 5, 6: at m = 6 A is the whole register; 8 RDMs in one call), 9 qubits (m = 1, 3, 4, 6:
   the tile is the state, both register branches); both solvers, B = 2 with shared and per-trajectory tables, 1 / 3 / 5 (padded) / 8
   directions.  Qubit lists are scrambled and hold qubit 0 and qubit N - 1 (the highest and the lowest index bit).
2. Past one tile (13 and 14 qubits, m = 1, 3, 6): duality with the native adjoint (k_rdm_apply) under a seeded cotangent over all
   rows, DUALITY_RTOL = 1e-9 of the larger side.
3. The RDM values of the tangent call against the RDM rows of evolve, 1e-10 (with 1 and 2).
4. Structure on the raw ABI: outputs and workspace NaN before the call, none afterwards; mirror entries exact conjugates, Im of the
   diagonal exactly 0.0; sum_a d rho[a][a] = the tangent row of the all-ones diagonal at 1e-12 relative; 5 and 7 directions equal
   the first 5 / 7 of an 8-direction call at 1e-12.
5. evolve_geometry(flags=TANGENT_RDMS): the same RDM tangent rows at 1e-12, the Gram matrix that of a call without RDMs.
6. XY kets: 4 qubits, PAIR_TERMS | RDMS, against tests.tangent_pair_reference at 1e-8.
7. Public route: the 6-atom chain, run_rdm_sensitivities(...).d_purity(0) at all times against the loop of reverse sweeps, 1e-9
   relative (PUBLIC_RTOL).

Measured on an MI355X (largest over the cases of each part): 1. tangents 3.9e-12 of the direction's largest entry, values 8.8e-14;
2. duality 1.2e-14, values against evolve 4.4e-16; 6. 6.8e-14 absolute; 7. 2.8e-14 relative.  The 9-qubit references take 3 to 6 s of
CPU each (two of the three are shared with tests/test_gpu_tangent_matrix.py); every other case runs below a second.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
import pulser_diff_amd.pulses as pl
from pulser_diff_amd import _native
from pulser_diff_amd import solver as S
from pulser_diff_amd.derivative import deriv_rdm_all_times
from pulser_diff_amd.observables import ReducedDensityMatrix
from pulser_diff_amd.solver import SolverType, evolve, evolve_geometry, evolve_tangent, split_observables
from pulser_diff_amd.utils import purity
from tests.helpers import random_terms, to_native
from tests.test_gpu_tangent import DUALITY_RTOL, ORACLE_RTOL, PUBLIC_RTOL, _randn
from tests.test_gpu_tangent_matrix import TSAVE, TSAVE_9, TSAVE_DP5_SHORT, _inputs, _problem, _reference

pytestmark = pytest.mark.gpu

VALUE_ATOL = 1e-9     # tests/test_gpu_rdm_observables.py
NATIVE_ATOL = 1e-10   # the tangent call's values against evolve's
RDMS = _native.TANGENT_RDMS

# scrambled qubit lists per register size; every list with two or more qubits holds qubit 0 and qubit N - 1, the single-qubit ones
# are those two
SUBSYSTEMS = {
    1: [(0,)],
    3: [(2,), (0,), (2, 0), (0, 2), (1, 2, 0)],
    6: [(5, 1, 0, 3), (2, 5, 0, 4, 1), (3, 5, 0, 4, 1, 2), (5,), (0,), (5, 0), (0, 3, 5), (4, 0, 5, 2)],  # 8 RDMs in one call
    9: [(8,), (0,), (8, 4, 0), (0, 8, 2, 5), (6, 0, 8, 3, 1, 7)],
}


def _partial(psi_a, psi_b, qubits, n):
    """Tr_E |a><b| for kets (..., dim, B) -> (..., B, 2^m, 2^m): qubit q is axis q of the (2,) * n index (qubit 0 most significant),
    the matrix index lists `qubits` with the first most significant."""
    lead = psi_a.shape[:-2]
    k, batch, m = len(lead), psi_a.shape[-1], len(qubits)
    rest = [q for q in range(n) if q not in qubits]
    order = list(range(k)) + [k + n] + [k + q for q in qubits] + [k + q for q in rest]
    shape = lead + (batch, 2**m, 2 ** (n - m))
    a = psi_a.reshape(lead + (2,) * n + (batch,)).permute(order).reshape(shape)
    b = psi_b.reshape(lead + (2,) * n + (batch,)).permute(order).reshape(shape)
    return torch.einsum("...ae,...ce->...ac", a, b.conj())


def _reference_rdms(ref, n, n_dir, subsystems):
    """(rho[o] (n_t, B, d, d), drho[o] (n_dir, n_t, B, d, d)) from the dense states (n_t, dim, B) and tangents (n_t, n_dir, dim, B)."""
    states, tangents = ref
    tang = tangents[:, :n_dir].permute(1, 0, 2, 3)  # (n_dir, n_t, dim, B)
    rho = [_partial(states, states, qs, n) for qs in subsystems]
    drho = []
    for qs in subsystems:
        half = _partial(tang, states[None].expand_as(tang), qs, n)
        drho.append(half + half.mH)
    return rho, drho


def _native_rdms(expect, dexpect, rdm_objs):
    rho = split_observables(expect.cpu(), 0, rdm_objs)[2]
    per_dir = [split_observables(dexpect[d].cpu(), 0, rdm_objs)[2] for d in range(dexpect.shape[0])]
    return rho, [torch.stack([per_dir[d][o] for d in range(len(per_dir))]) for o in range(len(rdm_objs))]


def _run(prob, solver_name, tsave, n_dir, subsystems, dev, which="adup", flags=RDMS, diag=None):
    _, _, _, spec = to_native(prob["terms"], dev, SolverType[solver_name], store_states=False)
    spec.rdms = [ReducedDensityMatrix(qs) for qs in subsystems]
    to_dev = lambda t: None if t is None else t.to(dev)  # noqa: E731
    d_amp, d_det, d_u, d_psi = (to_dev(t) for t in _inputs(prob, which, 0, n_dir))
    args = (prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), torch.tensor(tsave, dtype=torch.float64), prob["psi0"].to(dev), spec,
            to_dev(diag))
    return args, dict(d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi, flags=flags)


# ---- 1. entrywise against the dense oracle ---------------------------------------------------------------------------------------------
# (n, solver, coeff_batch, width of the shared reference, its save times, the direction counts sliced from it)
ORACLE_CASES = [
    (1, "KRYLOV_SE", 1, 8, TSAVE, (1, 8)),
    (1, "DP5_SE", 2, 8, TSAVE, (3, 5)),
    (3, "KRYLOV_SE", 2, 7, TSAVE, (1, 5)),      # the reference of tests/test_gpu_tangent_matrix.py's width tests
    (3, "DP5_SE", 1, 8, TSAVE, (3, 8)),
    (6, "KRYLOV_SE", 1, 8, TSAVE, (3, 8)),
    (6, "DP5_SE", 2, 8, TSAVE, (1, 5)),
    (9, "KRYLOV_SE", 2, 7, TSAVE_9, (3,)),      # tests/test_gpu_tangent_matrix.py's 7-direction reference, per-trajectory tables
    (9, "KRYLOV_SE", 1, 8, TSAVE_9, (1, 8)),
    (9, "DP5_SE", 1, 5, TSAVE_DP5_SHORT, (5,)),  # tests/test_gpu_tangent_matrix.py's padded-width reference
]
_ORACLE = [(n, s, cb, w, ts, d) for n, s, cb, w, ts, ds in ORACLE_CASES for d in ds]


@pytest.mark.parametrize("n,solver_name,cb,width,tsave,n_dir", _ORACLE, ids=[f"N{n}-{s}-cb{cb}-D{d}" for n, s, cb, _, _, d in _ORACLE])
def test_rdm_tangents_against_the_dense_oracle(n, solver_name, cb, width, tsave, n_dir, cuda_device):
    prob = _problem(n, 2, cb, width)
    ref = _reference(n, 2, cb, width, solver_name, tsave, "adup")
    subsystems = SUBSYSTEMS[n]
    args, tang = _run(prob, solver_name, tsave, n_dir, subsystems, cuda_device)
    expect, dexpect = evolve_tangent(*args, **tang)
    rows = sum(2 * 4 ** len(qs) for qs in subsystems)
    assert tuple(expect.shape) == (rows, len(tsave), 2) and tuple(dexpect.shape) == (n_dir, rows, len(tsave), 2)
    assert bool(torch.isfinite(expect).all()) and bool(torch.isfinite(dexpect).all())
    rdm_objs = args[5].rdms
    got_rho, got_drho = _native_rdms(expect, dexpect, rdm_objs)
    want_rho, want_drho = _reference_rdms(ref, n, n_dir, subsystems)
    dpsi_norm = ref[1][:, :n_dir].norm(dim=2).amax(dim=(0, 2))  # per direction: the largest ||dpsi_d(t_k)|| over times and trajectories
    for o, qs in enumerate(subsystems):
        val_err = float((got_rho[o] - want_rho[o]).abs().max())
        print(f"N{n} {solver_name} D{n_dir} A={qs}: values, max error {val_err:.2e}")
        assert tuple(got_drho[o].shape) == tuple(want_drho[o].shape)
        assert val_err <= VALUE_ATOL
        for d in range(n_dir):
            scale = float(want_drho[o][d].abs().max())
            err = float((got_drho[o][d] - want_drho[o][d]).abs().max())
            print(f"N{n} {solver_name} D{n_dir} A={qs} direction {d}: largest entry {scale:.3e}, max error {err:.3e} ({err / scale:.2e} relative)")
            assert scale > 1e-3 * float(dpsi_norm[d])  # nothing passes on zeros
            assert err <= ORACLE_RTOL * scale
    # 3. the values of the tangent call against evolve's RDM rows
    with torch.no_grad():
        _, plain = evolve(*args[:6], args[6])
    assert float((expect - plain).abs().max()) <= NATIVE_ATOL


# ---- 2. past one tile: duality with the native adjoint ------------------------------------------------------------------------------------
BIG_SUBSYSTEMS = {13: [(12,), (0, 12, 6), (7, 0, 12, 3, 9, 1)], 14: [(0,), (13, 5, 0), (2, 13, 0, 8, 11, 6)]}
# (n_qubits, solver, batch, coeff_batch, n_dir)
DUALITY_CASES = [(13, "KRYLOV_SE", 2, 2, 3), (13, "DP5_SE", 2, 1, 5), (14, "KRYLOV_SE", 1, 1, 2), (14, "DP5_SE", 2, 2, 1)]
BIG_SAMPLES, BIG_DT, BIG_TSAVE = 9, 0.004, (0.0, 0.0061, 0.0127, 0.0203)


@pytest.mark.parametrize("case", DUALITY_CASES, ids=[f"N{n}-{s}-B{b}-cb{cb}-D{d}" for n, s, b, cb, d in DUALITY_CASES])
def test_rdm_tangents_are_dual_to_the_native_adjoint(case, cuda_device):
    """sum w * dexpect_d == Re<g_amp, d_amp> + <g_det, d_det> + <g_u, d_u> + Re<g_psi0, d_psi0> with the g_* of
    evolve(...).backward under a seeded cotangent w over all rows: a diagonal row and the RDM blocks of m = 1, 3, 6 (2 or 4 tiles of
    2^12 amplitudes per state)."""
    n, solver_name, batch, cb, n_dir = case
    dev = cuda_device
    terms = random_terms(n, BIG_SAMPLES, BIG_DT, seed=1400 + n, local=True, phase=True)
    amp, det, u, spec = to_native(terms, dev, SolverType[solver_name], store_states=False, batch_tables=cb)
    gen = torch.Generator().manual_seed(81000 + 31 * n + 7 * n_dir + cb)
    if cb > 1:
        amp = amp * (1.0 + 0.1 * _randn(gen, cb, 1, 1).to(dev))
        det = det * (1.0 + 0.1 * _randn(gen, cb, 1, 1).to(dev))
    dim = 2**n
    psi0 = _randn(gen, batch, dim, cplx=True)
    psi0 = (psi0 / psi0.norm(dim=1, keepdim=True)).to(dev)
    spec.rdms = [ReducedDensityMatrix(qs) for qs in BIG_SUBSYSTEMS[n]]
    ones = torch.ones(1, dim, dtype=torch.float64, device=dev)
    tsave = torch.tensor(BIG_TSAVE, dtype=torch.float64)
    d_amp = (float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True)).to(dev)
    d_det = (float(det.abs().max()) * _randn(gen, n_dir, *det.shape)).to(dev)
    d_u = (float(u.abs().max()) * _randn(gen, n_dir, *u.shape)).to(dev)
    d_psi = (_randn(gen, n_dir, batch, dim, cplx=True) / np.sqrt(dim)).to(dev)
    expect_t, dexpect = evolve_tangent(amp, det, u, tsave, psi0, spec, ones, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi, flags=RDMS)
    leaves = [t.clone().requires_grad_(True) for t in (amp, det, u, psi0)]
    _, expect = evolve(leaves[0], leaves[1], leaves[2], tsave, leaves[3], spec, ones)
    rows = 1 + sum(2 * 4 ** len(qs) for qs in BIG_SUBSYSTEMS[n])
    assert tuple(expect.shape) == tuple(expect_t.shape) == (rows, len(BIG_TSAVE), batch) and tuple(dexpect.shape) == (n_dir,) + tuple(expect.shape)
    w = _randn(gen, *expect.shape).to(dev)
    (w * expect).sum().backward()
    g_amp, g_det, g_u, g_psi = (t.grad for t in leaves)
    for d in range(n_dir):
        prod = (w * dexpect[d]).double()
        lhs, abs_sum = float(prod.sum()), float(prod.abs().sum())
        rhs = (float((g_amp.conj() * d_amp[d]).real.sum()) + float((g_det * d_det[d]).sum()) + float((g_u * d_u[d]).sum())
               + float((g_psi.conj() * d_psi[d]).real.sum()))
        big = max(abs(lhs), abs(rhs))
        print(f"direction {d}: tangent {lhs:+.15e}  adjoint {rhs:+.15e}  rel {abs(lhs - rhs) / big:.2e}  big / sum|terms| {big / abs_sum:.2e}")
        assert big > 1e-3 * abs_sum > 0.0  # cannot pass on zeros
        assert abs(lhs - rhs) <= DUALITY_RTOL * big
    # 3. values
    verr = float((expect_t - expect.detach()).abs().max())
    print(f"max |expect(tangent) - expect(evolve)| = {verr:.2e}")
    assert float(expect.detach()[1:].abs().max()) > 1e-2
    assert verr <= NATIVE_ATOL


# ---- 4. structure, on the raw ABI -----------------------------------------------------------------------------------------------------
def _raw_tangent(args, tang, dev, fill):
    """rydiff_forward_tangent through the raw ABI, with expect_out, dexpect_out and the WHOLE workspace filled with `fill` before the
    call (the convention of tests/test_gpu_workspace_contents.py)."""
    amp, det, u, tsave, psi0, spec, diag = args
    L = _native.lib()
    call = S._Call(spec, amp.contiguous(), det.contiguous(), u.contiguous(), tsave.numpy(), psi0.shape[0], diag.contiguous())
    call.problem.kernel_variant = 0
    p = call.problem
    n_dir, n_t, batch = int(tang["d_amp"].shape[0]), len(tsave), psi0.shape[0]
    rows = p.n_obs + spec.rdm_rows()
    filled = lambda *shape: torch.full(shape, fill, dtype=torch.float64, device=dev)  # noqa: E731
    expect, dexpect = filled(rows, n_t, batch), filled(n_dir, rows, n_t, batch)
    bufs = [tang[k].contiguous() for k in ("d_amp", "d_det", "d_u", "d_psi0")]
    tg = _native.RydTangent()
    tg.n_dir, tg.flags = n_dir, tang["flags"]
    tg.d_amp, tg.d_det, tg.d_u, tg.d_psi0 = (b.data_ptr() for b in bufs)
    with torch.cuda.device(dev):
        stream = S._stream_ptr(dev)
        scratch = filled(_native.PLAN_SCRATCH_BYTES // 8).view(torch.uint8)
        info = _native.RydPlanInfo()
        _native.check(L.rydiff_plan(ctypes.byref(p), 0, 0, S._ptr(scratch), stream, ctypes.byref(info)))
        need = L.rydiff_tangent_workspace_bytes_flags(ctypes.byref(p), ctypes.byref(info), n_dir, tg.flags)
        assert need > 0, _native.last_error()
        workspace = filled((need + 7) // 8).view(torch.uint8)
        _native.check(L.rydiff_forward_tangent(ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), S._ptr(psi0.contiguous()),
                                               S._ptr(expect), S._ptr(dexpect), S._ptr(workspace), workspace.numel(), stream))
        torch.cuda.synchronize()
    return expect, dexpect


@lru_cache(maxsize=None)
def _structure_call(n, n_dir):
    dev = torch.device("cuda:0")
    prob = _problem(n, 2, 1, 8)
    ones = torch.ones(1, 2**n, dtype=torch.float64)
    args, tang = _run(prob, "KRYLOV_SE", TSAVE_9, n_dir, SUBSYSTEMS[n], dev, diag=ones)
    return args, _raw_tangent(args, tang, dev, float("nan"))


@pytest.mark.parametrize("n", [3, 9])
def test_structure_of_the_rdm_rows_with_poisoned_buffers(n, cuda_device):
    args, (expect, dexpect) = _structure_call(n, 8)
    assert bool(torch.isfinite(expect).all()) and bool(torch.isfinite(dexpect).all())  # no NaN left: every entry is written
    rdm_objs = args[5].rdms
    for label, rows in [("values", expect[1:])] + [(f"direction {d}", dexpect[d, 1:]) for d in range(8)]:
        mats = split_observables(rows, 0, [sum(1 << q for q in o.qubits) for o in rdm_objs])[2]  # (masks: the library's own order)
        for o, rho in enumerate(mats):
            assert torch.equal(rho, rho.mH), (label, o)  # mirror entries are exact conjugates
            assert float(torch.diagonal(rho, dim1=-2, dim2=-1).imag.abs().max()) == 0.0, (label, o)
    # the trace of d rho is the tangent of <psi|psi>: row 0, the all-ones diagonal
    for d in range(8):
        mats = split_observables(dexpect[d, 1:], 0, [sum(1 << q for q in o.qubits) for o in rdm_objs])[2]
        want = dexpect[d, 0]
        scale = float(want.abs().max())
        assert scale > 1e-3
        for o, drho in enumerate(mats):
            tr = torch.diagonal(drho, dim1=-2, dim2=-1).real.sum(-1)
            assert float((tr - want).abs().max()) <= 1e-12 * scale, (d, o)


@pytest.mark.parametrize("n_dir", [5, 7])
def test_padded_directions_leave_no_trace(n_dir, cuda_device):
    _, (expect8, dexpect8) = _structure_call(9, 8)
    _, (expect, dexpect) = _structure_call(9, n_dir)
    assert tuple(dexpect.shape) == (n_dir,) + tuple(expect8.shape)
    assert bool(torch.isfinite(dexpect).all())
    scale = float(dexpect8[:n_dir].abs().max())
    assert float((dexpect - dexpect8[:n_dir]).abs().max()) <= 1e-12 * scale
    assert float((expect - expect8).abs().max()) <= 1e-12


# ---- 5. the geometry entry ------------------------------------------------------------------------------------------------------------
def test_geometry_entry_returns_the_same_rdm_rows(cuda_device):
    prob = _problem(9, 2, 1, 8)
    args, tang = _run(prob, "KRYLOV_SE", TSAVE_9, 5, SUBSYSTEMS[9], cuda_device)
    expect_t, dexpect_t = evolve_tangent(*args, **tang)
    expect_g, dexpect_g, gram = evolve_geometry(*args, **tang)
    scale = float(dexpect_t.abs().max())
    assert scale > 1e-2 and tuple(dexpect_g.shape) == tuple(dexpect_t.shape)
    assert float((dexpect_g - dexpect_t).abs().max()) <= 1e-12 * scale
    assert float((expect_g - expect_t).abs().max()) <= 1e-12
    plain_args, plain_tang = _run(prob, "KRYLOV_SE", TSAVE_9, 5, [], cuda_device, flags=0)
    plain_args[5].rdms = None
    assert torch.equal(gram, evolve_geometry(*plain_args, **plain_tang)[2])  # (fixed-order sums: bit for bit)


# ---- 6. XY kets -----------------------------------------------------------------------------------------------------------------------
def test_rdm_tangents_with_pair_terms(cuda_device):
    from tests.test_gpu_tangent_pair_terms import _problem as pair_problem

    n, n_dir, dev = 4, 3, cuda_device
    prob = pair_problem(n, 3, "KRYLOV_SE", False)
    subsystems = [(3,), (0, 3), (3, 1, 0)]
    _, _, _, spec = to_native(prob["terms"], dev, SolverType.KRYLOV_SE, store_states=False)
    spec.pair_terms = prob["pairs"]
    spec.rdms = [ReducedDensityMatrix(qs) for qs in subsystems]
    sl = slice(0, n_dir)
    expect, dexpect = evolve_tangent(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), prob["tsave"], prob["psi0"].to(dev), spec, None,
                                     d_amp=prob["d_amp"][sl].to(dev), d_det=prob["d_det"][sl].to(dev), d_u=prob["d_u"][sl].to(dev),
                                     d_psi0=prob["d_psi"][sl].to(dev), flags=RDMS | _native.TANGENT_PAIR_TERMS)
    got_rho, got_drho = _native_rdms(expect, dexpect, spec.rdms)
    want_rho, want_drho = _reference_rdms(prob["ref"], n, n_dir, subsystems)
    for o in range(len(subsystems)):
        assert float((got_rho[o] - want_rho[o]).abs().max()) <= VALUE_ATOL
        for d in range(n_dir):
            scale = float(want_drho[o][d].abs().max())
            err = float((got_drho[o][d] - want_drho[o][d]).abs().max())
            print(f"XY A={subsystems[o]} direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
            assert scale > 1e-2
            assert err <= ORACLE_RTOL * scale


# ---- 7. public route ------------------------------------------------------------------------------------------------------------------
def _chain(dev, n_atoms=6):
    """The 6-atom chain of examples/entanglement_growth.py with a constant pulse behind the Blackman one, float64 parameters."""
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)  # noqa: E731
    area, omega, delta = f64([3.0]), f64([4.0]), f64([1.0])
    seq = pl.Sequence(pl.Register.rectangle(1, n_atoms, torch.tensor([7.0], dtype=torch.float64)), pl.MockDevice)
    seq.declare_channel("ch", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(400, area), pl.RampWaveform(400, -2.0, delta), 0), "ch")
    seq.add(pl.Pulse.ConstantPulse(200, omega, delta, 0.0), "ch")
    sim = P.TorchEmulator.from_sequence(seq, sampling_rate=0.1, evaluation_times=0.25, compute_device=dev)
    return sim, [omega, delta, area]


def test_public_route_equals_the_loop_of_reverse_sweeps(cuda_device):
    sim, x = _chain(cuda_device)
    obs = ReducedDensityMatrix((2, 0, 1))  # the left half of the chain, scrambled
    sens = deriv_rdm_all_times(sim, x, [obs, (5, 3)], solver=SolverType.KRYLOV_SE)
    n_t = len(sim.evaluation_times)
    assert [tuple(r.shape) for r in sens.rho] == [(n_t, 1, 8, 8), (n_t, 1, 4, 4)] and sens.rho[0].dtype == torch.complex128
    assert [[tuple(d.shape) for d in per] for per in sens.drho] == [[(n_t, 1, 8, 8, 1)] * 3, [(n_t, 1, 4, 4, 1)] * 3]
    assert tuple(sens.times.shape) == (n_t,)
    results = sim.run(solver=SolverType.KRYLOV_SE, observables=[obs], store_states=False)
    rho = results.reduced_density_matrix(obs)
    f = purity(rho)[:, 0]
    assert float((sens.rho[0].cpu() - rho.detach().cpu()).abs().max()) <= VALUE_ATOL
    assert float((sens.purity(0)[:, 0].cpu() - f.detach().cpu()).abs().max()) <= VALUE_ATOL
    want = [torch.stack([g[0] for g in rows]) for rows in
            zip(*[torch.autograd.grad(f[k], x, retain_graph=True) for k in range(n_t)])]  # per tensor of x: (n_t,)
    for name, got, ref in zip(("omega", "delta", "area"), sens.d_purity(0), want):
        assert tuple(got.shape) == (n_t, 1, 1)
        got, ref = got[:, 0, 0].cpu(), ref.detach().cpu().to(torch.float64)
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print(f"d purity / d {name}: largest entry {scale:.3e}, max error {err:.3e} ({err / scale:.2e} relative)")
        assert scale > 1e-3
        assert err <= PUBLIC_RTOL * scale
    assert tuple(sens.entropy(1).shape) == (n_t, 1) and [tuple(g.shape) for g in sens.d_entropy(1)] == [(n_t, 1, 1)] * 3
