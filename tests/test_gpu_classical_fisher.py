"""Classical Gram matrices of the tangent sweep on the GPU (rydiff_forward_fisher through pulser_diff_amd.solver.evolve_fisher and
through TorchEmulator.run_classical_fisher):  C_ij(t_k) = sum_y w_i[y] w_j[y],  w_0 = |psi|,  w_{1+d} = 2 Re(conj(psi / |psi|) dpsi_d).

A. Kernel parity on exact inputs: at k = 0 the matrix is that of the caller's psi0 / d_psi0, the reference is
   observables.classical_gram on the same tensors on the CPU.  Rounding only:
       |C_ij - C_ij^ref| <= (dim + 16) EPS sum_y e_i[y] e_j[y],     e_0 = |psi|,  e_{1+d} = 2 |dpsi_d|
   (any summation order plus the per-term rounding of w; the cancellation in Re(conj u dpsi) is bounded by the envelope).
B. Edge amplitudes at k = 0: magnitudes of 1e-170 (|psi|^2 underflows), exact zeros under O(1) tangents (the zero rule), a basis
   state with zero tangents.
C. Sweep parity at later times against tests.helpers.tangent_dense_reference (the cached problems of
   tests/test_gpu_tangent_matrix.py).  w is not smooth where |psi[y]| is small, so the bound is the first-order propagation of the
   project's entrywise bar, delta_i = ORACLE_RTOL |v_i| on every entry of v_i:
       |dw_0[y]| <= delta_0,    |dw_{1+d}[y]| <= 2 delta_{1+d} + 2 |dpsi_d[y]| min(2, 2 delta_0 / |psi[y]|)
       |C_ij - C_ij^ref| <= sum_y (|dw_i| e_j + e_i |dw_j| + |dw_i| |dw_j|)
   computed from the reference vectors; a case whose bound exceeds 1e-3 |w_i| |w_j| on any entry would be vacuous (asserted).
D. Contract: poisoned buffers, NULL dexpect_out / gram_out, bit reproducibility, gram_out = evolve_geometry's bits, exact symmetry,
   C_00 = G_00 and C_0d = 2 Re G_0d.
E. Analytic pins on one qubit, both solvers.   F. The public route.

Measured on an MI355X (largest error over the bound of its entry): A. at most 6.4e-2 of the bound (3 qubits, n_dir = 2; 9 qubits
2.3e-3, 19 qubits 8.3e-5); B. 3.0e-3 (tiny amplitudes), 3.2e-3 (exact zeros), the basis state exact; C. at most 1.5e-6 of the bound
(3 qubits KRYLOV_SE 1.5e-6, DP5_SE 6.0e-7, 9 qubits 7.6e-8 for both widths, 10 directions 6.7e-7), the bounds at most 1.4e-4 of
|w_i| |w_j| (9 qubits); D. C_00 = G_00 to the bit, C_0d - 2 Re G_0d 1.5e-4 of the bound; the poisoned, the NULL-output and the repeated
calls return the clean call's bits; E. detuning |F_C| <= 1.1e-26 against bars from 9.8e-12, drive |F_C - t^2| / t^2 <= 2.6e-13
(KRYLOV_SE), 3.1e-11 (DP5_SE, the same as F_Q's); F. lambda_min(F_Q - F_C) >= -3.4e-24 against bars down to -7.7e-13.
"""
import ctypes

import pytest
import torch

from pulser_diff_amd import _native
from pulser_diff_amd import solver as S
from pulser_diff_amd.derivative import classical_fisher_information_all_times, deriv_param_all_times, quantum_fisher_information_all_times
from pulser_diff_amd.geometry import MeasurementFisher, classical_fisher_information, fisher_efficiency, quantum_fisher_information
from pulser_diff_amd.observables import classical_gram
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve_fisher, evolve_geometry
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.helpers import to_native
from tests.test_gpu_geometry import PIN_DT, PIN_SAMPLES, PIN_TSAVE, _rows_problem
from tests.test_gpu_tangent import ORACLE_RTOL, _basic_usage, _randn
from tests.test_gpu_tangent_matrix import NATIVE_RTOL, TSAVE, TSAVE_9, _big_problem, _inputs, _problem, _reference

pytestmark = pytest.mark.gpu

EPS = float(torch.finfo(torch.float64).eps)


def _envelope_sums(psi, dpsi):
    """sum_y e_i[y] e_j[y] for psi (..., dim), dpsi (..., D, dim): (..., 1 + D, 1 + D)."""
    e = torch.cat([psi.abs()[..., None, :], 2.0 * dpsi.abs()], dim=-2)
    return torch.einsum("...iy,...jy->...ij", e, e)


# ---- A / B. k = 0: the matrix of the caller's vectors -------------------------------------------------------------------------------
def _tables(n, dev):
    """(amp, det, u, spec, one short save interval) of a cached problem of n qubits; B follows psi0."""
    if n == 19:
        terms, amp, det, u, _, _ = _big_problem("KRYLOV_SE", 1)
        tsave = (0.0, 0.0061)
    else:
        prob = _problem(n, 2, 1, 8)
        terms, amp, det, u = prob["terms"], prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev)
        tsave = TSAVE[:2]
    spec = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=False)[3]
    return amp, det, u, spec, torch.tensor(tsave, dtype=torch.float64)


def _check_initial(label, psi0, d_psi0, dev, floor=1e-2):
    """evolve_fisher on psi0 (B, dim), d_psi0 (D, B, dim): cgram[0] against classical_gram on the CPU, within A's bound."""
    n = psi0.shape[-1].bit_length() - 1
    amp, det, u, spec, tsave = _tables(n, dev)
    _, _, gram, cgram = evolve_fisher(amp, det, u, tsave, psi0.to(dev), spec, None, d_psi0=d_psi0.to(dev))
    n_dir, batch, dim = d_psi0.shape
    assert tuple(cgram.shape) == (2, batch, 1 + n_dir, 1 + n_dir) and cgram.dtype == torch.float64
    assert tuple(gram.shape) == tuple(cgram.shape) and gram.dtype == torch.complex128
    got = cgram.cpu()
    assert bool(torch.isfinite(got).all())  # both save points: no NaN or Inf
    assert torch.equal(got, got.transpose(-1, -2))
    tang = d_psi0.permute(1, 0, 2)  # (B, D, dim)
    want = classical_gram(psi0, tang)
    env = _envelope_sums(psi0, tang)
    bound = (dim + 16) * EPS * env
    err = (got[0] - want).abs()
    print(f"{label}: largest sum e_i e_j {float(env.max()):.3e}, largest |C - C_ref| {float(err.max()):.3e}, "
          f"largest error / bound {float((err / bound.clamp_min(1e-300)).max()):.2e}")
    assert float(env.max()) > floor  # nothing passes on zeros
    assert bool((err <= bound).all())
    return got[0], want


def _random_vectors(seed, n, batch, n_dir):
    gen = torch.Generator().manual_seed(seed)
    dim = 2**n
    psi0 = 1.3 * _randn(gen, batch, dim, cplx=True) / dim**0.5  # deliberately unnormalised
    d_psi0 = _randn(gen, n_dir, batch, dim, cplx=True) / dim**0.5
    return psi0, d_psi0


@pytest.mark.parametrize("n_dir", [1, 2, 3, 4, 5, 6, 7, 8])
def test_initial_matrix_every_width_at_three_qubits(n_dir, cuda_device):
    """8 amplitudes in a 256-thread block: the lanes past them contribute exact zeros.  Widths 5 and 7 run the kernels of 6 and 8."""
    psi0, d_psi0 = _random_vectors(3100 + n_dir, 3, 2, n_dir)
    _check_initial(f"A-N3-D{n_dir}", psi0, d_psi0, cuda_device)


@pytest.mark.parametrize("n_dir", [1, 5, 8])
def test_initial_matrix_at_nine_qubits(n_dir, cuda_device):
    """Two blocks per trajectory: the smallest shape with a cross-block sum."""
    psi0, d_psi0 = _random_vectors(9100 + n_dir, 9, 2, n_dir)
    _check_initial(f"A-N9-D{n_dir}", psi0, d_psi0, cuda_device)


def test_initial_matrix_at_nineteen_qubits(cuda_device):
    """2048 blocks' worth of amplitudes against the cap of 1024 blocks: every thread's stride loop makes two trips."""
    psi0, d_psi0 = _random_vectors(19100, 19, 1, 8)
    _check_initial("A-N19-D8", psi0, d_psi0, cuda_device)


def test_tiny_amplitudes(cuda_device):
    """A quarter of the amplitudes of psi0, and d_psi0 there, at magnitude 1e-170: |psi|^2 underflows, the contributions are about
    1e-340 and must come out as harmless zeros or denormals."""
    psi0, d_psi0 = _random_vectors(9201, 9, 2, 3)
    psi0[:, 1::4] *= 1e-170 / psi0[:, 1::4].abs()
    d_psi0[:, :, 1::4] *= 1e-170 / d_psi0[:, :, 1::4].abs()
    assert float(psi0[:, 1::4].abs().max()) < 1.1e-170
    _check_initial("B-tiny", psi0, d_psi0, cuda_device)


def test_exact_zero_amplitudes(cuda_device):
    """A quarter of the amplitudes exactly 0 under O(1) tangents: those indices contribute exactly nothing (the reference uses the
    zero rule) — the matrix is the one of the other three quarters."""
    psi0, d_psi0 = _random_vectors(9202, 9, 2, 3)
    psi0[:, 2::4] = 0.0
    d_psi0[:, :, 2::4] *= 2.0**4.5 * 5.0  # O(1) per entry
    assert float(d_psi0[:, :, 2::4].abs().mean()) > 0.5
    got, _ = _check_initial("B-zeros", psi0, d_psi0, cuda_device)
    dropped = d_psi0.clone()
    dropped[:, :, 2::4] = 0.0
    without = classical_gram(psi0, dropped.permute(1, 0, 2))
    bound = (512 + 16) * EPS * _envelope_sums(psi0, dropped.permute(1, 0, 2))
    assert bool(((got - without).abs() <= bound).all())


def test_basis_state_with_zero_tangents(cuda_device):
    psi0 = torch.zeros(2, 512, dtype=torch.complex128)
    psi0[0, 37] = 1.0
    psi0[1, 511] = 1.0
    got, _ = _check_initial("B-basis", psi0, torch.zeros(3, 2, 512, dtype=torch.complex128), cuda_device)
    # C = diag(1, 0, ...): C_00 within the bound (checked above), every other entry an exact zero
    got[:, 0, 0] = 0.0
    assert float(got.abs().max()) == 0.0


# ---- C. later times against the dense reference ------------------------------------------------------------------------------------
def _fisher(prob, solver_name, tsave, which, n_dir, dev, directions=None):
    idx = list(range(n_dir)) if directions is None else directions
    _, _, _, spec = to_native(prob["terms"], dev, SolverType[solver_name], store_states=False)
    to_dev = lambda t: None if t is None else t[idx].to(dev)  # noqa: E731
    d_amp, d_det, d_u, d_psi = (to_dev(t) for t in _inputs(prob, which, 0, None))
    return evolve_fisher(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), torch.tensor(tsave, dtype=torch.float64),
                         prob["psi0"].to(dev), spec, None, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi)


def _reference_vectors(ref, n_dir):
    """(psi (n_t, B, dim), dpsi (n_t, B, n_dir, dim)) of a dense reference."""
    states, tangents = ref
    return states.permute(0, 2, 1), tangents[:, :n_dir].permute(0, 3, 1, 2)


def _sweep_bound(psi, dpsi):
    """The first-order propagation of delta_i = ORACLE_RTOL |v_i| (module docstring, C) and the largest bound / (|w_i| |w_j|)."""
    mod = psi.abs()
    e = torch.cat([mod[..., None, :], 2.0 * dpsi.abs()], dim=-2)                     # (n_t, B, 1 + D, dim)
    delta = ORACLE_RTOL * torch.cat([psi.norm(dim=-1)[..., None], dpsi.norm(dim=-1)], dim=-1)  # (n_t, B, 1 + D)
    swing = torch.minimum(torch.full_like(mod, 2.0), 2.0 * delta[..., :1] / mod)      # min(2, 2 delta_0 / |psi[y]|); 2 at a zero
    dw = torch.cat([delta[..., :1, None].expand_as(mod[..., None, :]),
                    2.0 * delta[..., 1:, None] + 2.0 * dpsi.abs() * swing[..., None, :]], dim=-2)
    cross = torch.einsum("...iy,...jy->...ij", dw, e)
    bound = cross + cross.transpose(-1, -2) + torch.einsum("...iy,...jy->...ij", dw, dw)
    phase = torch.where(mod > 0, psi / mod.clamp_min(1e-300), torch.zeros_like(psi))
    w = torch.cat([mod[..., None, :], 2.0 * (phase.conj()[..., None, :] * dpsi).real], dim=-2)
    wn = w.norm(dim=-1)
    return bound, float((bound / (wn[..., :, None] * wn[..., None, :])).max())


def _check_sweep(label, cgram, ref, n_dir):
    psi, dpsi = _reference_vectors(ref, n_dir)
    want = classical_gram(psi, dpsi)
    bound, vacuity = _sweep_bound(psi, dpsi)
    got = cgram.cpu()
    assert tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all())
    err = (got - want).abs()
    print(f"{label}: largest |C - C_ref| {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.2e}, "
          f"largest bound / (|w_i| |w_j|) {vacuity:.2e}")
    assert vacuity <= 1e-3  # the bound says something on every entry
    assert float(want.abs().max()) > 1e-2
    assert bool((err <= bound).all())


@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_sweep_parity_at_three_qubits(solver_name, cuda_device):
    prob = _problem(3, 1, 1, 8)
    ref = _reference(3, 1, 1, 8, solver_name, TSAVE, "adup")
    _check_sweep(f"C-N3-{solver_name}-D8", _fisher(prob, solver_name, TSAVE, "adup", 8, cuda_device)[3], ref, 8)


@pytest.mark.parametrize("n_dir", [4, 5])
def test_sweep_parity_at_nine_qubits_krylov(n_dir, cuda_device):
    prob = _problem(9, 1, 1, 8)
    ref = _reference(9, 1, 1, 8, "KRYLOV_SE", TSAVE_9, "adup")
    _check_sweep(f"C-N9-KRYLOV-D{n_dir}", _fisher(prob, "KRYLOV_SE", TSAVE_9, "adup", n_dir, cuda_device)[3], ref, n_dir)


def test_ten_directions_in_three_sweeps(cuda_device):
    """10 directions = groups of 4, 4, 2 = three sweeps: the full 11 x 11 matrix, cross-group blocks included; the Gram matrix of the
    same call is evolve_geometry's."""
    prob = _problem(3, 2, 1, 13)
    ref = _reference(3, 2, 1, 13, "KRYLOV_SE", TSAVE_9, "ap")
    out = _fisher(prob, "KRYLOV_SE", TSAVE_9, "ap", 13, cuda_device, directions=list(range(10)))
    assert tuple(out[3].shape) == (len(TSAVE_9), 2, 11, 11)
    _check_sweep("C-N3-10-directions", out[3], ref, 10)
    assert torch.equal(out[3], out[3].transpose(-1, -2))


# ---- D. contract ---------------------------------------------------------------------------------------------------------------------
def _raw_fisher(args, tang, dev, fill, with_dexpect=True, with_gram=True):
    """rydiff_forward_fisher through the raw ABI, with cgram_out, gram_out, dexpect_out and the WHOLE workspace filled with `fill`
    before the call (the convention of tests/test_gpu_workspace_contents.py)."""
    amp, det, u, tsave, psi0, spec, diag = args
    L = _native.lib()
    call = S._Call(spec, amp.contiguous(), det.contiguous(), u.contiguous(), tsave.numpy(), psi0.shape[0], diag.contiguous())
    call.problem.kernel_variant = 0
    p = call.problem
    n_dir, n_t, batch = int(tang["d_amp"].shape[0]), len(tsave), psi0.shape[0]
    rows = p.n_obs + p.n_pauli_obs + 2 * p.n_overlaps
    filled = lambda *shape, dtype=torch.float64: torch.full(shape, fill, dtype=dtype, device=dev)  # noqa: E731
    cgram = filled(n_t, batch, 1 + n_dir, 1 + n_dir)
    gram = filled(n_t, batch, 1 + n_dir, 1 + n_dir, dtype=torch.complex128) if with_gram else None
    dexpect = filled(n_dir, rows, n_t, batch) if with_dexpect else None
    expect = filled(rows, n_t, batch)
    bufs = [tang[k].contiguous() for k in ("d_amp", "d_det", "d_u", "d_psi0")]
    tg = _native.RydTangent()
    tg.n_dir = n_dir
    tg.d_amp, tg.d_det, tg.d_u, tg.d_psi0 = (b.data_ptr() for b in bufs)
    with torch.cuda.device(dev):
        stream = S._stream_ptr(dev)
        scratch = filled(_native.PLAN_SCRATCH_BYTES // 8).view(torch.uint8)
        info = _native.RydPlanInfo()
        _native.check(L.rydiff_plan(ctypes.byref(p), 0, 0, S._ptr(scratch), stream, ctypes.byref(info)))
        need = L.rydiff_fisher_workspace_bytes_flags(ctypes.byref(p), ctypes.byref(info), n_dir, 0)
        assert need >= L.rydiff_geometry_workspace_bytes(ctypes.byref(p), ctypes.byref(info), n_dir) > 0
        workspace = filled((need + 7) // 8).view(torch.uint8)
        _native.check(L.rydiff_forward_fisher(ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), S._ptr(psi0.contiguous()),
                                              S._ptr(expect), S._ptr(dexpect), S._ptr(gram), S._ptr(cgram), S._ptr(workspace),
                                              workspace.numel(), stream))
        torch.cuda.synchronize()
    return expect, dexpect, gram, cgram


def _contract_problem(n_dir, dev):
    """The 9-qubit, B = 1 problem of the parity cases (its dense reference is cached) with rows, cut to n_dir directions."""
    _, args, tang = _rows_problem(9, 8, dev, batch=1)
    return args, {k: v[:n_dir] for k, v in tang.items()}


@pytest.mark.parametrize("n_dir", [5, 8])
def test_poisoned_buffers_null_outputs_and_reproducibility(n_dir, cuda_device):
    args, tang = _contract_problem(n_dir, cuda_device)
    clean = _raw_fisher(args, tang, cuda_device, 0.0)
    poisoned = _raw_fisher(args, tang, cuda_device, float("nan"))
    for a, b in zip(clean, poisoned):
        assert bool(torch.isfinite(torch.view_as_real(b) if b.is_complex() else b).all())
    assert float(clean[3].abs().max()) > 1e-2
    assert torch.equal(clean[3], poisoned[3]) and torch.equal(clean[2], poisoned[2])
    again = _raw_fisher(args, tang, cuda_device, float("nan"))
    assert torch.equal(again[3], clean[3]) and torch.equal(again[2], clean[2])  # two calls: the same bits
    bare = _raw_fisher(args, tang, cuda_device, float("nan"), with_dexpect=False, with_gram=False)
    assert bare[1] is None and bare[2] is None and torch.equal(bare[3], clean[3])
    no_gram = _raw_fisher(args, tang, cuda_device, float("nan"), with_gram=False)
    assert torch.equal(no_gram[3], clean[3])
    assert float((no_gram[1] - clean[1]).abs().max()) <= NATIVE_RTOL * float(clean[1].abs().max())  # (rows with atomics)
    # the Gram matrix of this call is evolve_geometry's, bit for bit; the public entry returns the raw call's bits
    assert torch.equal(clean[2], evolve_geometry(*args, **tang)[2])
    high = evolve_fisher(*args, **tang)
    assert torch.equal(high[2], clean[2]) and torch.equal(high[3], clean[3])
    assert torch.equal(clean[3], clean[3].transpose(-1, -2))  # exactly symmetric


def test_first_row_agrees_with_the_gram_matrix(cuda_device):
    """C_00 = G_00 to dim EPS (relative to S) and C_0d = 2 Re G_0d to A's bound, at every time; the envelopes of A's bound come from
    the dense reference's vectors (they are the sweep's to 1e-8)."""
    n_dir = 5
    args, tang = _contract_problem(n_dir, cuda_device)
    _, _, gram, cgram = evolve_fisher(*args, **tang)
    gram, cgram = gram.cpu(), cgram.cpu()
    s = gram[:, :, 0, 0].real
    d00 = (cgram[:, :, 0, 0] - s).abs()
    print(f"D: largest |C_00 - G_00| / (dim EPS S) {float((d00 / (512 * EPS * s)).max()):.2e}")
    assert bool((d00 <= 512 * EPS * s).all())
    psi, dpsi = _reference_vectors(_reference(9, 1, 1, 8, "KRYLOV_SE", TSAVE_9, "adup"), n_dir)
    bound = (512 + 16) * EPS * _envelope_sums(psi, dpsi)[:, :, 0, 1:]
    d0d = (cgram[:, :, 0, 1:] - 2.0 * gram[:, :, 0, 1:].real).abs()
    print(f"D: largest |C_0d - 2 Re G_0d| / bound {float((d0d / bound).max()):.2e}")
    assert float(gram[:, :, 0, 1:].real.abs().max()) > 1e-2
    assert bool((d0d <= bound).all())


# ---- E. analytic pins ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_detuning_pin(solver_name, cuda_device):
    """One qubit in |+> under a constant detuning (table -delta / 2), zero drive: d psi / d delta = i t n psi moves phases only, the
    distribution does not move: |F_C| <= ORACLE_RTOL t^2 while F_Q = 4 t^2 Var(n) = t^2 to the same bar."""
    dev = cuda_device
    spec = ProblemSpec(1, PIN_DT, PIN_SAMPLES, (1,), (1,), solver=SolverType[solver_name], store_states=False)
    amp = torch.zeros(1, 1, PIN_SAMPLES, dtype=torch.complex128, device=dev)
    det = torch.full((1, 1, PIN_SAMPLES), -0.5 * 3.7, dtype=torch.float64, device=dev)
    u = torch.zeros(0, dtype=torch.float64, device=dev)
    psi0 = torch.full((1, 2), 0.5**0.5, dtype=torch.complex128, device=dev)
    tsave = torch.tensor(PIN_TSAVE, dtype=torch.float64)
    _, _, gram, cgram = evolve_fisher(amp, det, u, tsave, psi0, spec, None,
                                      d_det=torch.full((1, 1, 1, PIN_SAMPLES), -0.5, dtype=torch.float64, device=dev))
    fc = classical_fisher_information(cgram)[:, 0, 0, 0].cpu()
    fq = quantum_fisher_information(gram)[:, 0, 0, 0].cpu()
    print(f"detuning pin {solver_name}: F_C {fc.tolist()}, F_Q {fq.tolist()} against t^2 {(tsave**2).tolist()}")
    assert bool((fc.abs() <= ORACLE_RTOL * tsave**2).all())
    assert bool(((fq - tsave**2).abs() <= ORACLE_RTOL * tsave**2).all())


@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_drive_pin(solver_name, cuda_device):
    """One qubit, constant resonant drive of phase 0 (table Omega / 2) from a basis state: p_1 = sin^2(Omega t / 2), so
    F_C = (d p_1)^2 / (p_0 p_1) = t^2 = F_Q: the occupation measurement saturates the bound — at times where sin(Omega t) is not
    within 1e-3 of 0 (there p_0 p_1 -> 0 and the ratio is 0 / 0; on this grid that is t = 0 alone, where F_C = 0 exactly)."""
    dev, omega = cuda_device, 6.3
    spec = ProblemSpec(1, PIN_DT, PIN_SAMPLES, (1,), (1,), solver=SolverType[solver_name], store_states=False)
    amp = torch.full((1, 1, PIN_SAMPLES), 0.5 * omega, dtype=torch.complex128, device=dev)
    det = torch.zeros(1, 1, PIN_SAMPLES, dtype=torch.float64, device=dev)
    u = torch.zeros(0, dtype=torch.float64, device=dev)
    tsave = torch.tensor(PIN_TSAVE, dtype=torch.float64)
    want = tsave**2
    regular = torch.sin(omega * tsave).abs() > 1e-3
    assert regular.tolist() == [False, True, True, True, True]
    for ground in (0, 1):
        psi0 = torch.zeros(1, 2, dtype=torch.complex128, device=dev)
        psi0[0, ground] = 1.0
        _, _, gram, cgram = evolve_fisher(amp, det, u, tsave, psi0, spec, None,
                                          d_amp=torch.full((1, 1, 1, PIN_SAMPLES), 0.5, dtype=torch.complex128, device=dev))
        fc = classical_fisher_information(cgram)[:, 0, 0, 0].cpu()
        fq = quantum_fisher_information(gram)[:, 0, 0, 0].cpu()
        print(f"drive pin {solver_name}: F_C {fc.tolist()}, F_Q {fq.tolist()} against t^2 {want.tolist()}")
        assert bool(((fc - want).abs() <= ORACLE_RTOL * want)[regular].all())
        assert bool(((fq - want).abs() <= ORACLE_RTOL * want)[regular].all())
        assert float(fc[0]) == 0.0
        eff = fisher_efficiency(cgram, gram)[:, 0, 0].cpu()
        assert bool(((eff - 1.0).abs() <= 2.0 * ORACLE_RTOL)[regular].all()) and bool(torch.isnan(eff[0]))


# ---- F. public route -------------------------------------------------------------------------------------------------------------------
def _psd_bar(gram, dim):
    """The sum of the rounding bounds of the entries of C, (dim + 16) EPS sum_y e_i e_j, with the envelope sums bounded through
    Cauchy-Schwarz by the norms the Gram matrix holds: |e_0|^2 = G_00, |e_{1+d}|^2 = 4 G_{1+d,1+d}.  (n_t,) or (n_t, B)."""
    norms = torch.diagonal(gram, dim1=-2, dim2=-1).real.clamp_min(0.0).sqrt()
    norms = torch.cat([norms[..., :1], 2.0 * norms[..., 1:]], dim=-1)
    return (dim + 16) * EPS * norms.sum(-1) ** 2


def test_public_route(cuda_device):
    sim, omega, area, coords = _basic_usage(cuda_device)
    x = [omega, area, coords["q0"]]
    obs = DiagonalObservable(total_magnetization_diag(4))
    out = classical_fisher_information_all_times(sim, x, observables=[obs])
    n_t = len(sim.evaluation_times)
    assert isinstance(out, MeasurementFisher) and out.route == "tangent"
    assert tuple(out.cfi.shape) == (n_t, 4, 4) and tuple(out.qfi.shape) == (n_t, 4, 4) and out.cfi.dtype == torch.float64
    assert tuple(out.cgram.shape) == (n_t, 5, 5) and tuple(out.gram.shape) == (n_t, 5, 5) and out.cgram.dtype == torch.float64
    assert float(out.cfi.abs().max()) > 1e-2
    assert torch.equal(out.cfi, out.cfi.transpose(-1, -2))
    # the deriv-level wrapper and the method return the same tensors
    direct = sim.run_classical_fisher(x, [obs])
    for name in ("cgram", "cfi", "gram", "qfi"):
        assert torch.equal(getattr(direct, name), getattr(out, name))
    # the quantum side is run_quantum_fisher's
    geo = quantum_fisher_information_all_times(sim, x, observables=[obs])
    assert torch.equal(out.qfi, geo.qfi) and torch.equal(out.gram, geo.gram)
    # values and grads: those of run_sensitivities
    sens = deriv_param_all_times(sim, x, [obs])
    assert out.values.shape == sens.values.shape and [g.shape for g in out.grads] == [g.shape for g in sens.grads]
    assert float((out.values - sens.values).abs().max()) <= NATIVE_RTOL * float(sens.values.abs().max())
    for got, want in zip(out.grads, sens.grads):
        assert float(want.abs().max()) > 1e-3
        assert float((got - want).abs().max()) <= NATIVE_RTOL * float(want.abs().max())
    # F_C <= F_Q as matrices at every time
    gap = (out.qfi - out.cfi).cpu()
    lam = torch.linalg.eigvalsh(0.5 * (gap + gap.transpose(-1, -2))).min(dim=-1).values
    bar = _psd_bar(out.gram.cpu(), 16)
    print(f"public route: smallest eigenvalue of F_Q - F_C {float(lam.min()):.3e}, smallest bar {-float(bar.max()):.3e}, "
          f"largest F_C / F_Q on the diagonal {float(torch.nan_to_num(fisher_efficiency(out.cgram, out.gram)).max()):.6f}")
    assert bool((lam >= -bar).all())
    # without observables: empty values and grads of the Sensitivities shapes
    bare = sim.run_classical_fisher(x)
    assert tuple(bare.values.shape) == (0, n_t) and [tuple(g.shape) for g in bare.grads] == [(0, n_t, 1), (0, n_t, 1), (0, n_t, 2)]
    assert torch.equal(bare.cfi, out.cfi)


def test_public_route_with_several_initial_columns(cuda_device):
    sim, omega, area, coords = _basic_usage(cuda_device, evaluation_times=0.25)
    x = [omega, coords["q0"]]
    single = sim.run_classical_fisher(x, solver=SolverType.KRYLOV_SE)
    gen = torch.Generator().manual_seed(777)
    cols = _randn(gen, 16, 2, cplx=True)
    cols = cols / cols.norm(dim=0, keepdim=True)
    cols[:, 0] = sim.initial_state[:, 0]
    sim.set_initial_state(cols)
    out = sim.run_classical_fisher(x, solver=SolverType.KRYLOV_SE)
    n_t = len(sim.evaluation_times)
    assert tuple(out.cfi.shape) == (n_t, 2, 3, 3) and tuple(out.qfi.shape) == (n_t, 2, 3, 3)
    assert tuple(out.cgram.shape) == (n_t, 2, 4, 4) and tuple(out.gram.shape) == (n_t, 2, 4, 4)
    # the geometry of a batch is per state: column 0 is the single run's
    assert float((out.cgram[:, 0] - single.cgram).abs().max()) <= NATIVE_RTOL * float(single.cgram.abs().max())
    gap = (out.qfi - out.cfi).cpu()
    lam = torch.linalg.eigvalsh(0.5 * (gap + gap.transpose(-1, -2))).min(dim=-1).values
    assert bool((lam >= -_psd_bar(out.gram.cpu(), 16)).all())


def test_no_live_tangent_gives_zeros_except_the_norm(cuda_device):
    """Tangents of inputs the problem does not have (d_u on one qubit): zeros, except C_00 = S = G_00."""
    dev = cuda_device
    spec = ProblemSpec(1, PIN_DT, PIN_SAMPLES, (1,), (1,), solver=SolverType.KRYLOV_SE, store_states=False)
    amp = torch.full((1, 1, PIN_SAMPLES), 0.5 * 6.3, dtype=torch.complex128, device=dev)
    det = torch.zeros(1, 1, PIN_SAMPLES, dtype=torch.float64, device=dev)
    u = torch.zeros(0, dtype=torch.float64, device=dev)
    psi0 = torch.tensor([[0.6, 0.8j], [1.5, 0.0]], dtype=torch.complex128, device=dev)
    tsave = torch.tensor(PIN_TSAVE, dtype=torch.float64)
    _, _, gram, cgram = evolve_fisher(amp, det, u, tsave, psi0, spec, None, d_u=torch.zeros(3, 0, dtype=torch.float64, device=dev))
    assert tuple(cgram.shape) == (len(PIN_TSAVE), 2, 4, 4) and cgram.dtype == torch.float64
    s = gram[..., 0, 0].real
    assert float((s[0].cpu() - torch.tensor([1.0, 2.25])).abs().max()) <= 8 * EPS
    assert bool(((cgram[..., 0, 0] - s).abs() <= 2 * EPS * s).all())
    rest = cgram.clone()
    rest[..., 0, 0] = 0.0
    assert float(rest.abs().max()) == 0.0 and float(classical_fisher_information(cgram).abs().max()) == 0.0
