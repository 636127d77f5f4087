"""Occupation-correlation tangents from the tangent sweep (k_moments_tangent, RYDIFF_TANGENT_MOMENTS): the moments S, B_q, B_qr of
the signed weight 2 Re(conj psi . dpsi_d) at every evaluation time, every direction.

1. Entry by entry against the dense forward-mode reference (tests.helpers.tangent_dense_reference; the rows formed here by a 0/1 bit
   table (rows, 2^N) times 2 Re(conj psi . dpsi_d)): values at VALUE_ATOL, tangents at ORACLE_RTOL of the direction's largest
   moment-tangent entry; per direction the largest single-row and the largest pair-row tangent must each exceed 1e-3 of
   max_k ||psi(t_k)|| max_k ||dpsi_d(t_k)|| (nothing passes on zeros; no floor on the S row, which can be 1e-4 of that scale).
   1 qubit (no pair rows), 2 (one pair), 3, 6 (one wave), 9 (the tile is the state, bits from N up masked out); both solvers, B = 2 with
   shared and per-trajectory tables, 1 / 3 / 5 (padded) / 8 directions.
2. One tile exactly and past it (12, 13, 14 qubits): the same call is handed diagonal tables for S, a low and a high single and
   low-low, high-low and (14) high-high pairs; native moment-tangent rows against those k_expect_tangent rows at ROUTE_TOL, and
   duality with the native adjoint (k_moments_apply) under a seeded cotangent over all rows at DUALITY_RTOL.
3. The Moments block of the tangent call's values against evolve's, 1e-10 (with 1 and 2).
4. Structure on the raw ABI (9 and 13 qubits): outputs and workspace NaN before the call, none afterwards; the dS row equals the
   tangent row of the all-ones diagonal at 1e-12 relative; 5 and 7 directions equal the first 5 / 7 of an 8-direction call at 1e-12.
5. Two calls on the same input: bit-identical Moments blocks of dexpect (9 and 13 qubits).
6. evolve_geometry(flags=TANGENT_MOMENTS): the same rows at 1e-12, dS_d = 2 Re gram[0, 1 + d] at 1e-12 relative, the Gram matrix
   bit-identical to a call without moments.
7. TANGENT_MOMENTS | TANGENT_RDMS on the problem of tests/test_gpu_row_layout.py: every block where ExpectRows puts it, the moment
   rows unchanged by the RDM rows' presence.
8. XY kets: 4 qubits, PAIR_TERMS | MOMENTS, against tests.tangent_pair_reference at 1e-8.
9. Public route: the 6-atom chain of tests/test_gpu_rdm_tangent.py, run_occupation_sensitivities(...).d_structure_factor(neel) and
   d_correlations(connected=True) at all times against the loop of one-hot reverse sweeps, PUBLIC_RTOL.

Tolerances are the project's own; every use names its source line.

Measured on an MI355X (largest over the cases of each part): 1. tangents 2.5e-12 of the direction's largest entry, values 1.0e-13;
the smallest single-row / pair-row tangent over that scale 9.0e-3; 2. native rows against diagonal-table rows 8.8e-16 of the largest,
duality 3.7e-15; 3. values against evolve 1.1e-15; 7. 2.3e-13 absolute; 8. 1.2e-13 absolute; 9. 7.7e-14 relative, values 3.6e-15.
The 9-qubit references take 3 to 5 s of CPU each (all three are shared with tests/test_gpu_tangent_matrix.py or
tests/test_gpu_rdm_tangent.py); every other case runs below 1.5 s.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

from pulser_diff_amd import _native
from pulser_diff_amd import solver as S
from pulser_diff_amd.derivative import deriv_occupations_all_times
from pulser_diff_amd.observables import OccupationCorrelations, moment_rows
from pulser_diff_amd.solver import SolverType, evolve, evolve_geometry, evolve_tangent, split_moments
from tests.helpers import random_terms, to_native
from tests.test_gpu_occupation_moments import _moment_row_of, _picked_bits, _tables
from tests.test_gpu_rdm_observables import ROUTE_TOL  # :27
from tests.test_gpu_rdm_tangent import _chain
from tests.test_gpu_tangent import DUALITY_RTOL, ORACLE_RTOL, PUBLIC_RTOL, _randn  # :31, :33, :34
from tests.test_gpu_tangent_matrix import TSAVE, TSAVE_9, TSAVE_DP5_SHORT, VALUE_ATOL, _inputs, _problem, _reference  # VALUE_ATOL :53

pytestmark = pytest.mark.gpu

NATIVE_ATOL = 1e-10   # the tangent call's values against evolve's (tests/test_gpu_rdm_tangent.py:48)
MOMENTS = _native.TANGENT_MOMENTS


def _bit_table(n):
    """(1 + N + N(N-1)/2, 2^N) of 0 / 1: the all-ones row, y_q (qubit q <-> index bit N-1-q) in ascending q, y_q y_r in
    lexicographic (q, r)."""
    y = torch.arange(2 ** n)
    bit = [((y >> (n - 1 - q)) & 1).to(torch.float64) for q in range(n)]
    rows = [torch.ones(2 ** n, dtype=torch.float64)] + bit + [bit[q] * bit[r] for q in range(n) for r in range(q + 1, n)]
    return torch.stack(rows)


def _reference_moments(ref, n, n_dir):
    """(moments (rows, n_t, B), dmoments (n_dir, rows, n_t, B)) from the dense states (n_t, dim, B) and tangents (n_t, n_dir, dim, B)."""
    states, tangents = ref
    table = _bit_table(n)
    p = states.real ** 2 + states.imag ** 2
    dp = 2.0 * (states.conj()[:, None] * tangents[:, :n_dir]).real  # (n_t, n_dir, dim, B)
    return torch.einsum("ry,kyb->rkb", table, p), torch.einsum("ry,kdyb->drkb", table, dp)


def _run(prob, solver_name, tsave, n_dir, dev, which="adup", flags=MOMENTS, diag=None, moments=True):
    _, _, _, spec = to_native(prob["terms"], dev, SolverType[solver_name], store_states=False)
    spec.moments = moments
    to_dev = lambda t: None if t is None else t.to(dev)  # noqa: E731
    d_amp, d_det, d_u, d_psi = (to_dev(t) for t in _inputs(prob, which, 0, n_dir))
    args = (prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), torch.tensor(tsave, dtype=torch.float64), prob["psi0"].to(dev), spec,
            to_dev(diag))
    return args, dict(d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi, flags=flags)


# ---- 1. entrywise against the dense oracle ---------------------------------------------------------------------------------------------
# (n, solver, coeff_batch, width of the shared reference, its save times, the direction counts sliced from it); the 9-qubit
# references are those of tests/test_gpu_tangent_matrix.py and tests/test_gpu_rdm_tangent.py
ORACLE_CASES = [
    (1, "KRYLOV_SE", 1, 8, TSAVE, (1, 8)),
    (1, "DP5_SE", 2, 8, TSAVE, (3, 5)),
    (2, "KRYLOV_SE", 2, 8, TSAVE, (3, 5)),
    (2, "DP5_SE", 1, 8, TSAVE, (1, 8)),
    (3, "KRYLOV_SE", 2, 7, TSAVE, (1, 5)),
    (3, "DP5_SE", 1, 8, TSAVE, (3, 8)),
    (6, "KRYLOV_SE", 1, 8, TSAVE, (3, 8)),
    (6, "DP5_SE", 2, 8, TSAVE, (1, 5)),
    (9, "KRYLOV_SE", 2, 7, TSAVE_9, (3,)),
    (9, "KRYLOV_SE", 1, 8, TSAVE_9, (1, 8)),
    (9, "DP5_SE", 1, 5, TSAVE_DP5_SHORT, (5,)),
]
_ORACLE = [(n, s, cb, w, ts, d) for n, s, cb, w, ts, ds in ORACLE_CASES for d in ds]


@pytest.mark.parametrize("n,solver_name,cb,width,tsave,n_dir", _ORACLE, ids=[f"N{n}-{s}-cb{cb}-D{d}" for n, s, cb, _, _, d in _ORACLE])
def test_moment_tangents_against_the_dense_oracle(n, solver_name, cb, width, tsave, n_dir, cuda_device):
    prob = _problem(n, 2, cb, width)
    ref = _reference(n, 2, cb, width, solver_name, tsave, "adup")
    args, tang = _run(prob, solver_name, tsave, n_dir, cuda_device)
    expect, dexpect = evolve_tangent(*args, **tang)
    rows = moment_rows(n)
    assert tuple(expect.shape) == (rows, len(tsave), 2) and tuple(dexpect.shape) == (n_dir, rows, len(tsave), 2)
    assert bool(torch.isfinite(expect).all()) and bool(torch.isfinite(dexpect).all())
    want_val, want_der = _reference_moments(ref, n, n_dir)
    got_val, got_der = expect.cpu(), dexpect.cpu()
    val_err = float((got_val - want_val).abs().max())
    print(f"MOMENT-TANGENT N{n} {solver_name} cb{cb} D{n_dir}: values, max error {val_err:.2e}")
    assert val_err <= VALUE_ATOL  # tests/test_gpu_tangent_matrix.py:53
    psi_norm = float(ref[0].norm(dim=1).max())
    dpsi_norm = ref[1][:, :n_dir].norm(dim=2).amax(dim=(0, 2))  # per direction: the largest ||dpsi_d(t_k)|| over times and trajectories
    for d in range(n_dir):
        scale = float(want_der[d].abs().max())
        err = float((got_der[d] - want_der[d]).abs().max())
        singles = float(want_der[d, 1:1 + n].abs().max())
        pairs = float(want_der[d, 1 + n:].abs().max()) if n > 1 else None
        floor = 1e-3 * psi_norm * float(dpsi_norm[d])
        print(f"MOMENT-TANGENT N{n} {solver_name} cb{cb} D{n_dir} direction {d}: largest entry {scale:.3e}, max error {err:.3e} "
              f"({err / scale:.2e} relative); largest single {singles:.2e}, pair {pairs if pairs is None else format(pairs, '.2e')}, floor {floor:.2e}")
        assert singles > floor and (pairs is None or pairs > floor)  # nothing passes on zeros
        assert err <= ORACLE_RTOL * scale  # tests/test_gpu_tangent.py:33
    # 3. the values of the tangent call against evolve's Moments block
    with torch.no_grad():
        _, plain = evolve(*args[:6], args[6])
    assert float((expect - plain).abs().max()) <= NATIVE_ATOL


# ---- 2. one tile exactly and past it: the diagonal-table route and duality with the native adjoint -----------------------------------
# (n_qubits, solver, batch, coeff_batch, n_dir)
BIG_CASES = [(12, "KRYLOV_SE", 2, 1, 2), (13, "KRYLOV_SE", 2, 2, 3), (13, "DP5_SE", 2, 1, 5), (14, "KRYLOV_SE", 1, 1, 2), (14, "DP5_SE", 1, 1, 1)]
BIG_SAMPLES, BIG_DT, BIG_TSAVE = 9, 0.004, (0.0, 0.0061, 0.0127)  # two save intervals


@pytest.mark.parametrize("case", BIG_CASES, ids=[f"N{n}-{s}-B{b}-cb{cb}-D{d}" for n, s, b, cb, d in BIG_CASES])
def test_moment_tangents_against_diagonal_tables_and_the_native_adjoint(case, cuda_device):
    """One tangent call is handed the diagonal tables of tests/test_gpu_occupation_moments.py's picked bits — S, the lowest and the
    highest index bit, two lane bits (low-low), a lane bit with the highest bit (high-low past one tile), the two highest bits
    (high-low at 13: one high bit and no high-high pair; high-high at 14), a wave bit with a thread bit — next to the Moments block.
    Then sum w * dexpect_d == Re<g_amp, d_amp> + <g_det, d_det> + <g_u, d_u> + Re<g_psi0, d_psi0> with the g_* of
    evolve(...).backward under a seeded cotangent w over all rows."""
    n, solver_name, batch, cb, n_dir = case
    dev = cuda_device
    terms = random_terms(n, BIG_SAMPLES, BIG_DT, seed=1500 + n, local=True, phase=True)
    amp, det, u, spec = to_native(terms, dev, SolverType[solver_name], store_states=False, batch_tables=cb)
    gen = torch.Generator().manual_seed(83000 + 31 * n + 7 * n_dir + cb)
    if cb > 1:
        amp = amp * (1.0 + 0.1 * _randn(gen, cb, 1, 1).to(dev))
        det = det * (1.0 + 0.1 * _randn(gen, cb, 1, 1).to(dev))
    dim = 2 ** n
    psi0 = _randn(gen, batch, dim, cplx=True)
    psi0 = (1.3 * psi0 / psi0.norm(dim=1, keepdim=True)).to(dev)  # not normalised: the S row matters
    spec.moments = True
    tables = _tables(n, dev)
    picked = _picked_bits(n)
    tsave = torch.tensor(BIG_TSAVE, dtype=torch.float64)
    d_amp = (float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True)).to(dev)
    d_det = (float(det.abs().max()) * _randn(gen, n_dir, *det.shape)).to(dev)
    d_u = (float(u.abs().max()) * _randn(gen, n_dir, *u.shape)).to(dev)
    d_psi = (_randn(gen, n_dir, batch, dim, cplx=True) / np.sqrt(dim)).to(dev)
    expect_t, dexpect = evolve_tangent(amp, det, u, tsave, psi0, spec, tables, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi, flags=MOMENTS)
    rows = len(picked) + moment_rows(n)
    assert tuple(expect_t.shape) == (rows, len(BIG_TSAVE), batch) and tuple(dexpect.shape) == (n_dir,) + tuple(expect_t.shape)
    assert bool(torch.isfinite(dexpect).all())
    native_rows = [_moment_row_of(n, bits) for bits in picked]
    for d in range(n_dir):
        diag_rows, mom = split_moments(dexpect[d], n)
        scale = float(diag_rows.abs().max())
        err = float((mom[native_rows] - diag_rows).abs().max())
        print(f"MOMENT-TANGENT N{n} {solver_name} direction {d}: native rows against diagonal-table rows, largest entry {scale:.3e}, "
              f"max difference {err:.3e} ({err / scale:.2e} relative)")
        assert scale > 1e-3
        assert err <= ROUTE_TOL * scale  # tests/test_gpu_rdm_observables.py:27
    # duality with the native adjoint
    leaves = [t.clone().requires_grad_(True) for t in (amp, det, u, psi0)]
    _, expect = evolve(leaves[0], leaves[1], leaves[2], tsave, leaves[3], spec, tables)
    w = _randn(gen, *expect.shape).to(dev)
    w[:len(picked)] = 0.0  # the Moments block alone: the diagonal rows' duality is tests/test_gpu_tangent.py's
    (w * expect).sum().backward()
    g_amp, g_det, g_u, g_psi = (t.grad for t in leaves)
    for d in range(n_dir):
        prod = (w * dexpect[d]).double()
        lhs, abs_sum = float(prod.sum()), float(prod.abs().sum())
        rhs = (float((g_amp.conj() * d_amp[d]).real.sum()) + float((g_det * d_det[d]).sum()) + float((g_u * d_u[d]).sum())
               + float((g_psi.conj() * d_psi[d]).real.sum()))
        big = max(abs(lhs), abs(rhs))
        print(f"MOMENT-TANGENT N{n} {solver_name} direction {d}: tangent {lhs:+.15e}  adjoint {rhs:+.15e}  rel {abs(lhs - rhs) / big:.2e}  "
              f"big / sum|terms| {big / abs_sum:.2e}")
        assert big > 1e-3 * abs_sum > 0.0  # cannot pass on zeros
        assert abs(lhs - rhs) <= DUALITY_RTOL * big  # tests/test_gpu_tangent.py:31
    # 3. values
    verr = float((expect_t - expect.detach()).abs().max())
    print(f"MOMENT-TANGENT N{n} {solver_name}: max |expect(tangent) - expect(evolve)| = {verr:.2e}")
    assert float(expect.detach()[len(picked):].abs().max()) > 1e-2
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
    rows = call.expect_rows()
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


def _big_problem(n, n_dir=8):
    """A seeded 13-qubit-style problem in the shape of _problem's (which builds no reference): B = 2, shared tables."""
    terms = random_terms(n, BIG_SAMPLES, BIG_DT, seed=1600 + n, local=True, phase=True)
    amp, det, u, _ = to_native(terms, "cpu", SolverType.KRYLOV_SE)
    gen = torch.Generator().manual_seed(84000 + n)
    dim = 2 ** n
    psi0 = _randn(gen, 2, dim, cplx=True)
    return {"terms": terms, "amp": amp, "det": det, "u": u, "psi0": psi0 / psi0.norm(dim=1, keepdim=True),
            "d_amp": float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True),
            "d_det": float(det.abs().max()) * _randn(gen, n_dir, *det.shape),
            "d_u": float(u.abs().max()) * _randn(gen, n_dir, *u.shape),
            "d_psi0": _randn(gen, n_dir, 2, dim, cplx=True) / np.sqrt(dim)}


@lru_cache(maxsize=None)
def _structure_call(n, n_dir):
    dev = torch.device("cuda:0")
    prob, tsave = (_problem(n, 2, 1, 8), TSAVE_9) if n <= 9 else (_big_problem(n), BIG_TSAVE)
    ones = torch.ones(1, 2 ** n, dtype=torch.float64)
    args, tang = _run(prob, "KRYLOV_SE", tsave, n_dir, dev, diag=ones)
    return args, tang, _raw_tangent(args, tang, dev, float("nan"))


@pytest.mark.parametrize("n", [9, 13])
def test_structure_of_the_moment_rows_with_poisoned_buffers(n, cuda_device):
    _, _, (expect, dexpect) = _structure_call(n, 8)
    assert tuple(dexpect.shape) == (8, 1 + moment_rows(n), expect.shape[1], 2)
    assert bool(torch.isfinite(expect).all()) and bool(torch.isfinite(dexpect).all())  # no NaN left: every entry is written
    for d in range(8):  # dS is the tangent of <psi|psi>: row 0, the all-ones diagonal
        want, got = dexpect[d, 0], dexpect[d, 1]
        scale = float(want.abs().max())
        assert scale > 1e-3
        assert float((got - want).abs().max()) <= 1e-12 * scale, d


@pytest.mark.parametrize("n", [9, 13])
@pytest.mark.parametrize("n_dir", [5, 7])
def test_padded_directions_leave_no_trace(n, n_dir, cuda_device):
    _, _, (expect8, dexpect8) = _structure_call(n, 8)
    _, _, (expect, dexpect) = _structure_call(n, n_dir)
    assert tuple(dexpect.shape) == (n_dir,) + tuple(expect8.shape)
    assert bool(torch.isfinite(dexpect).all())
    scale = float(dexpect8[:n_dir].abs().max())
    assert scale > 1e-3
    assert float((dexpect - dexpect8[:n_dir]).abs().max()) <= 1e-12 * scale
    assert float((expect - expect8).abs().max()) <= 1e-12


# ---- 5. bit-reproducibility -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 13])
def test_two_calls_return_bit_identical_moment_tangents(n, cuda_device):
    args, tang, (_, first) = _structure_call(n, 8)
    _, second = _raw_tangent(args, tang, cuda_device, float("nan"))
    assert torch.equal(first[:, 1:], second[:, 1:])
    assert float(first[:, 1:].abs().max()) > 1e-3


# ---- 6. the geometry entry ------------------------------------------------------------------------------------------------------------
def test_geometry_entry_returns_the_same_moment_rows(cuda_device):
    prob = _problem(9, 2, 1, 8)
    args, tang = _run(prob, "KRYLOV_SE", TSAVE_9, 5, cuda_device)
    expect_t, dexpect_t = evolve_tangent(*args, **tang)
    expect_g, dexpect_g, gram = evolve_geometry(*args, **tang)
    scale = float(dexpect_t.abs().max())
    assert scale > 1e-2 and tuple(dexpect_g.shape) == tuple(dexpect_t.shape)
    assert float((dexpect_g - dexpect_t).abs().max()) <= 1e-12 * scale
    assert float((expect_g - expect_t).abs().max()) <= 1e-12
    for d in range(5):  # dS_d = 2 Re <psi|dpsi_d>
        want = 2.0 * gram[:, :, 0, 1 + d].real
        ds = float(want.abs().max())
        assert ds > 1e-3
        assert float((dexpect_g[d, 0] - want).abs().max()) <= 1e-12 * ds
    plain_args, plain_tang = _run(prob, "KRYLOV_SE", TSAVE_9, 5, cuda_device, flags=0, moments=False)
    assert torch.equal(gram, evolve_geometry(*plain_args, **plain_tang)[2])  # (fixed-order sums: bit for bit)


# ---- 7. next to every other ket block ---------------------------------------------------------------------------------------------------
def test_moments_and_rdms_in_one_tangent_call(cuda_device):
    """The ket problem of tests/test_gpu_row_layout.py (4 qubits, B = 2; 6 real rows, RDMs of 8 + 32 rows) with the 11 moment rows behind
    the RDM block: rows 0..45 equal the call without moments bit for bit or to 1e-12 (the RDM rows are summed with atomics), the
    Moments block equals that of a call with moments alone, and both match the dense reference."""
    from tests.helpers import tangent_dense_reference
    from tests.test_gpu_row_layout import BATCH, N, N_DIR, N_REAL, _ket_call

    dev = cuda_device
    prob = _problem(N, BATCH, 1, N_DIR)
    tsave = torch.tensor(TSAVE_9, dtype=torch.float64)
    d_amp, d_det, d_u, d_psi = _inputs(prob, "adup", 0, N_DIR)
    ref = tangent_dense_reference(prob["ref_terms"], d_amp[:, 0], d_det[:, 0], d_u, prob["psi0"].T.contiguous(), d_psi.permute(0, 2, 1).contiguous(),
                                  tsave, SolverType.KRYLOV_SE)
    want_val, want_der = _reference_moments(ref, N, N_DIR)
    spec, diag_dev = _ket_call(prob, dev)
    run = lambda sp, dg, flags: evolve_tangent(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), tsave, prob["psi0"].to(dev), sp, dg,  # noqa: E731
                                               d_amp=d_amp.to(dev), d_det=d_det.to(dev), d_u=d_u.to(dev), d_psi0=d_psi.to(dev), flags=flags)
    without, dwithout = run(spec, diag_dev, _native.TANGENT_RDMS)
    spec.moments = True
    expect, dexpect = run(spec, diag_dev, _native.TANGENT_RDMS | MOMENTS)
    front = N_REAL + 8 + 32
    assert moment_rows(N) == 11
    assert tuple(expect.shape) == (front + 11, len(tsave), BATCH) and tuple(dexpect.shape) == (N_DIR,) + tuple(expect.shape)
    assert torch.equal(expect[:N_REAL], without[:N_REAL]) and torch.equal(dexpect[:, :N_REAL], dwithout[:, :N_REAL])
    assert float((expect[N_REAL:front] - without[N_REAL:]).abs().max()) <= 1e-12
    assert float((dexpect[:, N_REAL:front] - dwithout[:, N_REAL:]).abs().max()) <= 1e-12 * float(dwithout[:, N_REAL:].abs().max())
    _, _, _, alone = to_native(prob["terms"], dev, SolverType.KRYLOV_SE, store_states=False)
    alone.moments = True
    expect_a, dexpect_a = run(alone, None, MOMENTS)
    assert torch.equal(expect[front:], expect_a) and torch.equal(dexpect[:, front:], dexpect_a)  # unchanged by the RDM rows' presence
    assert float((expect[front:].cpu() - want_val).abs().max()) <= VALUE_ATOL  # tests/test_gpu_tangent_matrix.py:53
    for d in range(N_DIR):
        scale, err = float(want_der[d].abs().max()), float((dexpect[d, front:].cpu() - want_der[d]).abs().max())
        print(f"MOMENT-TANGENT every block: direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
        assert scale > 1e-2
        assert err <= ORACLE_RTOL * scale  # tests/test_gpu_tangent.py:33


# ---- 8. XY kets -----------------------------------------------------------------------------------------------------------------------
def test_moment_tangents_with_pair_terms(cuda_device):
    from tests.test_gpu_tangent_pair_terms import _problem as pair_problem

    n, n_dir, dev = 4, 3, cuda_device
    prob = pair_problem(n, 3, "KRYLOV_SE", False)
    _, _, _, spec = to_native(prob["terms"], dev, SolverType.KRYLOV_SE, store_states=False)
    spec.pair_terms = prob["pairs"]
    spec.moments = True
    sl = slice(0, n_dir)
    expect, dexpect = evolve_tangent(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), prob["tsave"], prob["psi0"].to(dev), spec, None,
                                     d_amp=prob["d_amp"][sl].to(dev), d_det=prob["d_det"][sl].to(dev), d_u=prob["d_u"][sl].to(dev),
                                     d_psi0=prob["d_psi"][sl].to(dev), flags=MOMENTS | _native.TANGENT_PAIR_TERMS)
    want_val, want_der = _reference_moments(prob["ref"], n, n_dir)
    assert float((expect.cpu() - want_val).abs().max()) <= VALUE_ATOL  # tests/test_gpu_tangent_matrix.py:53
    for d in range(n_dir):
        scale = float(want_der[d].abs().max())
        err = float((dexpect[d].cpu() - want_der[d]).abs().max())
        print(f"MOMENT-TANGENT XY direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
        assert scale > 1e-2
        assert err <= ORACLE_RTOL * scale  # 1e-8: tests/test_gpu_tangent.py:33


# ---- 9. public route ------------------------------------------------------------------------------------------------------------------
def test_public_route_equals_the_loop_of_reverse_sweeps(cuda_device):
    sim, x = _chain(cuda_device)
    neel = [1, -1, 1, -1, 1, -1]
    sens = deriv_occupations_all_times(sim, x, solver=SolverType.KRYLOV_SE)
    n_t = len(sim.evaluation_times)
    assert tuple(sens.moments.shape) == (moment_rows(6), n_t, 1) and sens.occupied_bit == 0
    assert [tuple(d.shape) for d in sens.dmoments] == [(moment_rows(6), n_t, 1, 1)] * 3 and tuple(sens.times.shape) == (n_t,)
    results = sim.run(solver=SolverType.KRYLOV_SE, observables=[OccupationCorrelations()], store_states=False)
    f = results.structure_factor(neel)                        # (n_t,)
    g = results.occupation_correlations(connected=True)       # (n_t, 6, 6)
    for name, got, want in (("structure factor", sens.structure_factor(neel)[:, 0], f), ("connected correlations", sens.correlations(True)[:, 0], g),
                            ("occupations", sens.occupations()[:, 0], results.occupations())):
        scale, err = float(want.detach().abs().max()), float((got.cpu() - want.detach().cpu()).abs().max())
        print(f"MOMENT-TANGENT public {name}: largest entry {scale:.3e}, against run() {err:.3e}")
        assert scale > 1e-3 and err <= PUBLIC_RTOL * scale  # tests/test_gpu_tangent.py:34
    # the loop the sweep replaces: one reverse sweep per evaluation time and scalar
    want_f = [torch.stack([gr[0] for gr in rows]) for rows in zip(*[torch.autograd.grad(f[k], x, retain_graph=True) for k in range(n_t)])]
    picked = [(i, j) for i in range(6) for j in range(i, 6)]  # the upper triangle with the diagonal: g is symmetric (checked below)
    want_g = {ij: [torch.stack([gr[0] for gr in rows]) for rows in zip(*[torch.autograd.grad(g[k, ij[0], ij[1]], x, retain_graph=True) for k in range(n_t)])]
              for ij in picked}
    got_f, got_g = sens.d_structure_factor(neel), sens.d_correlations(connected=True)
    assert [tuple(t.shape) for t in got_f] == [(n_t, 1, 1)] * 3 and [tuple(t.shape) for t in got_g] == [(n_t, 1, 6, 6, 1)] * 3
    assert [tuple(t.shape) for t in sens.d_occupations()] == [(n_t, 1, 6, 1)] * 3
    for i, name in enumerate(("omega", "delta", "area")):
        # every entry of d g against the largest one of the matrix and parameter, as the oracle tests hold a direction's rows: an
        # entry between distant atoms can be far below the products <n_i> d<n_j> it is the difference of
        want = torch.zeros(n_t, 6, 6, dtype=torch.float64)
        for (a, b), per_x in want_g.items():
            want[:, a, b] = want[:, b, a] = per_x[i].detach().cpu().to(torch.float64)
        checks = [("d structure factor", got_f[i][:, 0, 0], want_f[i].detach().cpu().to(torch.float64)), ("d g", got_g[i][:, 0, :, :, 0], want)]
        for label, got, ref in checks:
            scale, err = float(ref.abs().max()), float((got.cpu() - ref).abs().max())
            print(f"MOMENT-TANGENT public {label} / d {name}: largest entry {scale:.3e}, max error {err:.3e} ({err / scale:.2e} relative)")
            assert scale > 1e-3
            assert err <= PUBLIC_RTOL * scale  # tests/test_gpu_tangent.py:34
    for i in range(3):  # the matrix of derivatives is symmetric like g itself
        assert float((got_g[i] - got_g[i].transpose(2, 3)).abs().max()) <= 1e-12
