"""Gram matrices of the tangent sweep on the GPU (rydiff_forward_geometry through pulser_diff_amd.solver.evolve_geometry and through
TorchEmulator.run_quantum_fisher):  G_ij(t_k) = <v_i|v_j>,  v_0 = psi,  v_{1+d} = dpsi_d.

A. Entrywise parity with the dense forward-mode reference of tests/test_gpu_tangent_matrix.py (tests.helpers.tangent_dense_reference;
   the problems and references are that module's cached ones, so a reference is computed once per session).  The reference Gram is an
   einsum over its states and tangent states.  Bound:  |G_ij - G_ij^ref| <= 2 * ORACLE_RTOL * |v_i| |v_j|  with reference norms —
   ORACLE_RTOL = 1e-8 is the project's bar for the tangent states against this oracle, the factor 2 is bilinearity.
B. Layout, poisoned buffers, bit reproducibility, consistency with evolve_tangent.
C. 19 qubits: 2^19 amplitudes are 2048 blocks of 256 against k_tangent_gram's grid of at most 1024 blocks, so every thread's stride loop
   makes two trips.  No dense oracle there: (a) unitarity and (b) norm conservation, exact references that do not come from the code
   under test.
D. Analytic pins (closed forms) and the public route.

Measured on an MI355X (largest error over the bound of its entry): A. at most 2.0e-5 of the bound over all parity cases (10 directions
at 3 qubits; 9 qubits KRYLOV_SE 3.0e-6, DP5_SE 4.2e-7); C. unitarity 1.9e-6 of the bound, |Re G_0d| 1.2e-14 against a bound of 1e-8;
the poisoned, the NULL-dexpect and the repeated call return the clean call's bits.  The reference CPU time is that of
tests/test_gpu_tangent_matrix.py's references (the DP5_SE one here: about 4.5 s).
"""
import ctypes

import numpy as np
import pytest
import torch

from pulser_diff_amd import _native
from pulser_diff_amd import solver as S
from pulser_diff_amd.derivative import deriv_param_all_times, quantum_fisher_information_all_times
from pulser_diff_amd.geometry import berry_curvature, quantum_fisher_information, quantum_geometric_tensor
from pulser_diff_amd.observables import StateOverlap, pack_overlaps
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, evolve_geometry, evolve_tangent
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.helpers import to_native
from tests.test_gpu_tangent import ORACLE_RTOL, _basic_usage, _randn, observable_set
from tests.test_gpu_tangent_matrix import (NATIVE_RTOL, TSAVE, TSAVE_9, TSAVE_DP5_SHORT, BIG_TSAVE, N_BIG, _big_problem, _inputs, _problem,
                                           _reference)

pytestmark = pytest.mark.gpu

EPS = float(torch.finfo(torch.float64).eps)


def _torch_gram(vectors):
    """(..., n, dim) -> (..., n, n): conj on the left index."""
    return torch.einsum("...iy,...jy->...ij", vectors.conj(), vectors)


def _geometry(prob, solver_name, tsave, which, n_dir, dev, directions=None):
    idx = list(range(n_dir)) if directions is None else directions
    _, _, _, spec = to_native(prob["terms"], dev, SolverType[solver_name], store_states=False)
    to_dev = lambda t: None if t is None else t[idx].to(dev)  # noqa: E731
    d_amp, d_det, d_u, d_psi = (to_dev(t) for t in _inputs(prob, which, 0, None))
    return evolve_geometry(prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), torch.tensor(tsave, dtype=torch.float64),
                           prob["psi0"].to(dev), spec, None, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi)[2]


def _check_gram(label, gram, ref, n_dir):
    """Every entry of gram (n_t, B, 1 + n_dir, 1 + n_dir) against the Gram matrix of the reference's states and tangent states."""
    states, tangents = ref
    v = torch.cat([states[:, None], tangents[:, :n_dir]], dim=1).permute(0, 3, 1, 2)  # (n_t, B, 1 + n_dir, dim)
    want = _torch_gram(v)
    norms = v.norm(dim=-1)
    bound = 2.0 * ORACLE_RTOL * norms[..., :, None] * norms[..., None, :]
    got = gram.cpu()
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.complex128
    assert bool(torch.isfinite(torch.view_as_real(got)).all())
    err = (got - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{label}: smallest |v_i| at the last time {float(norms[-1].min()):.3e}, largest |G - G_ref| {float(err.max()):.3e}, "
          f"largest error / bound {worst:.2e}")
    assert float(norms[-1].min()) > 1e-2  # nothing passes on zeros
    assert bool((err <= bound).all())


# ---- A. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dir", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_widths_at_three_qubits(solver_name, n_dir, cuda_device):
    """3 qubits, every instantiated width: 8 amplitudes are less than one wave, the lanes past them contribute exact zeros."""
    prob = _problem(3, 1, 1, 8)
    ref = _reference(3, 1, 1, 8, solver_name, TSAVE, "adup")
    _check_gram(f"N3-{solver_name}-D{n_dir}", _geometry(prob, solver_name, TSAVE, "adup", n_dir, cuda_device), ref, n_dir)


@pytest.mark.parametrize("n_dir", [1, 4, 8, 5, 7])
def test_widths_at_nine_qubits_krylov(n_dir, cuda_device):
    """9 qubits = two blocks per trajectory: the smallest shape with a cross-block sum.  Widths 5 and 7 run the kernels of 6 and 8 with
    a zero direction: the output has 1 + n_dir rows (the shape check of _check_gram) and no trace of the padded one."""
    prob = _problem(9, 1, 1, 8)
    ref = _reference(9, 1, 1, 8, "KRYLOV_SE", TSAVE_9, "adup")
    _check_gram(f"N9-KRYLOV-D{n_dir}", _geometry(prob, "KRYLOV_SE", TSAVE_9, "adup", n_dir, cuda_device), ref, n_dir)


def test_padded_width_at_nine_qubits_dp5(cuda_device):
    """9 qubits, DP5_SE, 7 directions (the kernels of 8), B = 1, three CF4 pieces: a reference of its own (about 5 s of CPU)."""
    prob = _problem(9, 1, 1, 7)
    ref = _reference(9, 1, 1, 7, "DP5_SE", TSAVE_DP5_SHORT, "adup")
    _check_gram("N9-DP5-D7", _geometry(prob, "DP5_SE", TSAVE_DP5_SHORT, "adup", 7, cuda_device), ref, 7)


@pytest.mark.parametrize("cb", [1, 3])
def test_batch_shapes_at_three_qubits(cb, cuda_device):
    """B = 3, shared and per-trajectory tables, d_psi0 given: every trajectory against its own reference column."""
    prob = _problem(3, 3, cb, 2)
    ref = _reference(3, 3, cb, 2, "KRYLOV_SE", TSAVE, "adup")
    gram = _geometry(prob, "KRYLOV_SE", TSAVE, "adup", 2, cuda_device)
    _check_gram(f"N3-B3-cb{cb}", gram, ref, 2)
    assert float((gram[:, 0] - gram[:, 1]).abs().max()) > 1e-3  # the trajectories do differ


@pytest.mark.parametrize("which", ["a", "d", "u", "p"])
def test_single_inputs_at_nine_qubits(which, cuda_device):
    prob = _problem(9, 2, 1, 5)
    ref = _reference(9, 2, 1, 5, "KRYLOV_SE", TSAVE_9, which)
    _check_gram(f"N9-only-{which}", _geometry(prob, "KRYLOV_SE", TSAVE_9, which, 5, cuda_device), ref, 5)


def test_ten_directions_in_three_sweeps(cuda_device):
    """10 directions = groups of 4, 4, 2 = three sweeps: the full 11 x 11 matrix, cross-group blocks included."""
    prob = _problem(3, 2, 1, 13)
    ref = _reference(3, 2, 1, 13, "KRYLOV_SE", TSAVE_9, "ap")
    gram = _geometry(prob, "KRYLOV_SE", TSAVE_9, "ap", 13, cuda_device, directions=list(range(10)))
    assert tuple(gram.shape) == (len(TSAVE_9), 2, 11, 11)
    _check_gram("N3-10-directions", gram, ref, 10)


# ---- B. layout, buffers, reproducibility, consistency -------------------------------------------------------------------------------------
def _rows_problem(n, n_dir, dev, batch=2):
    """The 8-direction problem of the width tests with a diagonal row, the Pauli set and one overlap."""
    prob = _problem(n, batch, 1, n_dir)
    _, _, _, spec = to_native(prob["terms"], dev, SolverType.KRYLOV_SE, store_states=False)
    spec.pauli = observable_set(n)
    spec.overlaps = pack_overlaps([StateOverlap(prob["targets_shared"][0])], 2**n, batch, dev)
    args = (prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), torch.tensor(TSAVE_9, dtype=torch.float64), prob["psi0"].to(dev),
            spec, prob["diags"][:1].to(dev))
    tang = dict(d_amp=prob["d_amp"].to(dev), d_det=prob["d_det"].to(dev), d_u=prob["d_u"].to(dev), d_psi0=prob["d_psi0"].to(dev))
    return prob, args, tang


def test_layout(cuda_device):
    prob, args, tang = _rows_problem(9, 5, cuda_device)
    _, _, gram = evolve_geometry(*args, **tang)
    assert torch.equal(gram, gram.transpose(-1, -2).conj())  # the lower triangle is the exact conjugate of the upper one
    assert float(torch.diagonal(gram, dim1=-2, dim2=-1).imag.abs().max()) == 0.0
    spec_s = to_native(prob["terms"], cuda_device, SolverType.KRYLOV_SE, store_states=True)[3]
    with torch.no_grad():
        states, _ = evolve(args[0], args[1], args[2], args[3], args[4], spec_s)  # (n_t, B, dim)
    norm2 = (states.conj() * states).real.sum(-1)
    assert float((gram[:, :, 0, 0].real - norm2).abs().max()) <= 1e-12
    # k = 0: the Gram matrix of (psi0, d_psi0); both sides sum 512 products of float64 in some order: (dim + 2) eps |v_i| |v_j| each
    v0 = torch.cat([args[4][None], tang["d_psi0"]]).permute(1, 0, 2)  # (B, 1 + D, dim)
    want = _torch_gram(v0)
    norms = v0.norm(dim=-1)
    bound = 2.0 * (v0.shape[-1] + 2) * EPS * norms[:, :, None] * norms[:, None, :]
    assert bool(((gram[0] - want).abs() <= bound).all())


def _raw_geometry(args, tang, dev, with_dexpect, fill):
    """rydiff_forward_geometry through the raw ABI, with gram_out, dexpect_out and the WHOLE workspace filled with `fill` before
    the call (the convention of tests/test_gpu_workspace_contents.py)."""
    amp, det, u, tsave, psi0, spec, diag = args
    L = _native.lib()
    call = S._Call(spec, amp.contiguous(), det.contiguous(), u.contiguous(), tsave.numpy(), psi0.shape[0], diag.contiguous())
    call.problem.kernel_variant = 0
    p = call.problem
    n_dir, n_t, batch = int(tang["d_amp"].shape[0]), len(tsave), psi0.shape[0]
    rows = p.n_obs + p.n_pauli_obs + 2 * p.n_overlaps
    filled = lambda *shape, dtype=torch.float64: torch.full(shape, fill, dtype=dtype, device=dev)  # noqa: E731
    gram = filled(n_t, batch, 1 + n_dir, 1 + n_dir, dtype=torch.complex128)
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
        need = L.rydiff_geometry_workspace_bytes(ctypes.byref(p), ctypes.byref(info), n_dir)
        assert need >= L.rydiff_tangent_workspace_bytes(ctypes.byref(p), ctypes.byref(info), n_dir) > 0
        workspace = filled((need + 7) // 8).view(torch.uint8)
        _native.check(L.rydiff_forward_geometry(ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), S._ptr(psi0.contiguous()),
                                                S._ptr(expect), S._ptr(dexpect), S._ptr(gram), S._ptr(workspace), workspace.numel(), stream))
        torch.cuda.synchronize()
    return expect, dexpect, gram


@pytest.mark.parametrize("n,n_dir", [(3, 5), (9, 5), (9, 8)])
def test_poisoned_buffers_and_null_dexpect(n, n_dir, cuda_device):
    """gram_out, dexpect_out and the whole workspace NaN before the call: the output is finite everywhere and bit for bit the clean
    call's; without dexpect_out (NULL) the Gram matrix is the same bits again."""
    _, args, tang = _rows_problem(n, n_dir, cuda_device)
    clean = _raw_geometry(args, tang, cuda_device, True, 0.0)
    poisoned = _raw_geometry(args, tang, cuda_device, True, float("nan"))
    for a, b in zip(clean, poisoned):
        assert bool(torch.isfinite(torch.view_as_real(b) if b.is_complex() else b).all())
    assert float(clean[2].abs().min()) > 0.0
    assert torch.equal(clean[2], poisoned[2])
    no_rows = _raw_geometry(args, tang, cuda_device, False, float("nan"))
    assert no_rows[1] is None and torch.equal(no_rows[2], clean[2])
    assert float((no_rows[0] - clean[0]).abs().max()) <= NATIVE_RTOL * float(clean[0].abs().max())  # (rows with atomics)


def test_two_calls_are_bit_identical(cuda_device):
    _, args, tang = _rows_problem(9, 8, cuda_device)
    first = evolve_geometry(*args, **tang)[2]
    second = evolve_geometry(*args, **tang)[2]
    assert torch.equal(first, second)


def test_rows_agree_with_evolve_tangent(cuda_device):
    _, args, tang = _rows_problem(9, 5, cuda_device)
    expect, dexpect, _ = evolve_geometry(*args, **tang)
    want_e, want_d = evolve_tangent(*args, **tang)
    assert expect.shape == want_e.shape and dexpect.shape == want_d.shape and dexpect.numel() > 0
    assert float(want_e.abs().max()) > 1e-2 and float(want_d.abs().max()) > 1e-2
    assert float((expect - want_e).abs().max()) <= NATIVE_RTOL * float(want_e.abs().max())
    for d in range(dexpect.shape[0]):
        assert float((dexpect[d] - want_d[d]).abs().max()) <= NATIVE_RTOL * float(want_d[d].abs().max())


# ---- C. 19 qubits -----------------------------------------------------------------------------------------------------------------
def test_nineteen_qubits_unitarity_and_norm_conservation(cuda_device):
    """2^19 amplitudes = 2048 blocks of 256 against the grid of at most 1024: the stride loop of k_tangent_gram makes two trips.
    D = 2, two save intervals, B = 1.  (a) Only d_psi0: the tangents evolve by the same unitary as psi, G(t_k) = G(t_0), the Gram
    matrix torch forms from psi0 and d_psi0; |dG_ij| <= 2 ORACLE_RTOL |v_i| |v_j|.  (b) Hermitian table tangents (d_det, real d_amp):
    Re G_0d = d<psi|psi>/d theta_d / 2 = 0; |Re G_0d| <= 2 ORACLE_RTOL |dpsi_d| with |psi| = 1 and |dpsi_d| = sqrt(G_dd)."""
    dev = cuda_device
    terms, amp, det, u, spec, psi0 = _big_problem("KRYLOV_SE", 1)
    spec = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=False)[3]
    gen = torch.Generator().manual_seed(190021)
    dim, n_dir = 2**N_BIG, 2
    tsave = torch.tensor(BIG_TSAVE, dtype=torch.float64)
    # (a) tangents with weight on psi0 as well, so that no entry of G is small against its bound's scale
    d_psi = torch.stack([complex(_randn(gen, 1, cplx=True)) * psi0 + (_randn(gen, 1, dim, cplx=True) / np.sqrt(dim)).to(dev)
                         for _ in range(n_dir)])
    gram = evolve_geometry(amp, det, u, tsave, psi0, spec, None, d_psi0=d_psi)[2]
    v0 = torch.cat([psi0[None], d_psi]).permute(1, 0, 2)  # (1, 3, dim)
    want = _torch_gram(v0)
    norms = v0.norm(dim=-1)
    bound = 2.0 * ORACLE_RTOL * norms[:, :, None] * norms[:, None, :]
    assert tuple(gram.shape) == (3, 1, 3, 3) and float(want.abs().min()) > 1e-2
    for k in range(3):
        err = (gram[k] - want).abs()
        print(f"N19 unitarity, k = {k}: largest |G - G(t_0)| {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.2e}")
        assert bool((err <= bound).all())
    # (b)
    d_amp = (float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape)).to(torch.complex128).to(dev)
    d_det = (float(det.abs().max()) * _randn(gen, n_dir, *det.shape)).to(dev)
    gram = evolve_geometry(amp, det, u, tsave, psi0, spec, None, d_amp=d_amp, d_det=d_det)[2]
    dnorm = gram[:, 0].diagonal(dim1=-2, dim2=-1).real[:, 1:].sqrt()  # (n_t, D)
    re = gram[:, 0, 0, 1:].real
    print(f"N19 norm conservation: |dpsi_d| {dnorm[-1].tolist()}, |Re G_0d| {re.abs().amax(0).tolist()}, "
          f"|Im G_0d| {gram[-1, 0, 0, 1:].imag.abs().tolist()}")
    assert float(dnorm[-1].min()) > 1e-3  # the tangents are there
    assert bool((re.abs() <= 2.0 * ORACLE_RTOL * dnorm).all())


# ---- D. analytic pins -------------------------------------------------------------------------------------------------------------
PIN_SAMPLES, PIN_DT = 41, 0.004
PIN_TSAVE = (0.0, 0.0313, 0.0622, 0.0951, 0.1513)


@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_detuning_pin(solver_name, cuda_device):
    """Zero drive, the uniform superposition on 4 qubits, one global detuning term (table -delta / 2), interactions on: everything is
    diagonal and commutes, d psi / d delta = i t (sum_j n_j) psi, so F(t_k) = 4 t_k^2 Var(sum_j n_j) = n t_k^2 and the Berry
    curvature (one parameter) is 0.  1e-8 relative to t_k^2."""
    dev, n = cuda_device, 4
    spec = ProblemSpec(n, PIN_DT, PIN_SAMPLES, (2**n - 1,), (2**n - 1,), solver=SolverType[solver_name], store_states=False)
    amp = torch.zeros(1, 1, PIN_SAMPLES, dtype=torch.complex128, device=dev)
    det = torch.full((1, 1, PIN_SAMPLES), -0.5 * 3.7, dtype=torch.float64, device=dev)
    u = torch.tensor([2.1, 0.4, 1.3, 0.9, 0.2, 3.0], dtype=torch.float64, device=dev)
    psi0 = torch.full((1, 2**n), 0.25, dtype=torch.complex128, device=dev)
    tsave = torch.tensor(PIN_TSAVE, dtype=torch.float64)
    gram = evolve_geometry(amp, det, u, tsave, psi0, spec, None, d_det=torch.full((1, 1, 1, PIN_SAMPLES), -0.5, dtype=torch.float64, device=dev))[2]
    f = quantum_fisher_information(gram)[:, 0, 0, 0].cpu()
    want = n * tsave**2
    print(f"detuning pin {solver_name}: F {f.tolist()} against n t^2 {want.tolist()}")
    assert bool(((f - want).abs() <= ORACLE_RTOL * tsave**2).all())
    # one parameter: -2 Im Q_11 = 2 Im(G_10 G_01) / N^2, zero up to the rounding of one complex product: the same bar
    assert bool((berry_curvature(gram)[:, 0, 0, 0].abs().cpu() <= ORACLE_RTOL * tsave**2).all())


@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
def test_drive_pin(solver_name, cuda_device):
    """One qubit, constant resonant drive of phase 0 (table Omega / 2), psi0 = |g>: psi = exp(-i Omega t sigma_x / 2)|g>,
    d psi / d Omega = -i (t / 2) sigma_x psi, <sigma_x> = 0, so F(t_k) = t_k^2.  1e-8 relative to t_k^2."""
    dev = cuda_device
    spec = ProblemSpec(1, PIN_DT, PIN_SAMPLES, (1,), (1,), solver=SolverType[solver_name], store_states=False)
    amp = torch.full((1, 1, PIN_SAMPLES), 0.5 * 6.3, dtype=torch.complex128, device=dev)
    det = torch.zeros(1, 1, PIN_SAMPLES, dtype=torch.float64, device=dev)
    u = torch.zeros(0, dtype=torch.float64, device=dev)
    tsave = torch.tensor(PIN_TSAVE, dtype=torch.float64)
    want = tsave**2
    for ground in (0, 1):  # F is the same from either basis state: the pin does not lean on which index is |g>
        psi0 = torch.zeros(1, 2, dtype=torch.complex128, device=dev)
        psi0[0, ground] = 1.0
        gram = evolve_geometry(amp, det, u, tsave, psi0, spec, None,
                               d_amp=torch.full((1, 1, 1, PIN_SAMPLES), 0.5, dtype=torch.complex128, device=dev))[2]
        f = quantum_fisher_information(gram)[:, 0, 0, 0].cpu()
        print(f"drive pin {solver_name}: F {f.tolist()} against t^2 {want.tolist()}")
        assert bool(((f - want).abs() <= ORACLE_RTOL * want).all())


# ---- D. public route --------------------------------------------------------------------------------------------------------------
def test_public_route(cuda_device):
    sim, omega, area, coords = _basic_usage(cuda_device)
    x = [omega, area, coords["q0"]]
    obs = DiagonalObservable(total_magnetization_diag(4))
    geo = quantum_fisher_information_all_times(sim, x, observables=[obs])
    n_t = len(sim.evaluation_times)
    assert geo.route == "tangent" and tuple(geo.qfi.shape) == (n_t, 4, 4) and tuple(geo.gram.shape) == (n_t, 5, 5)
    assert tuple(geo.qgt.shape) == (n_t, 4, 4) and tuple(geo.berry.shape) == (n_t, 4, 4) and geo.qfi.dtype == torch.float64
    scale = float(geo.qfi.abs().max())
    assert scale > 1e-2
    assert float((geo.qfi - geo.qfi.transpose(-1, -2)).abs().max()) <= 1e-10 * scale
    assert float(torch.linalg.eigvalsh(0.5 * (geo.qfi + geo.qfi.transpose(-1, -2))).min()) >= -1e-10 * scale
    # the same tangents through the low-level entry: the same bits (fixed-order sums)
    ham = sim._hamiltonian
    d_amp, d_det, d_u = sim._table_tangents(x)
    psi0 = sim.initial_state
    psi_bd = psi0.reshape(psi0.shape[0], -1).transpose(0, 1).to(cuda_device)
    spec = ham.problem_spec(solver=SolverType.DP5_SE, tol=S.tolerance_from_options({}), store_states=False)
    gram = evolve_geometry(ham.amp_tables, ham.det_tables, ham.u_pairs, sim.evaluation_times.detach(), psi_bd, spec, None,
                           d_amp=d_amp, d_det=d_det, d_u=d_u)[2]
    assert torch.equal(quantum_fisher_information(gram)[:, 0], geo.qfi)
    assert torch.equal(quantum_geometric_tensor(geo.gram), geo.qgt)
    # values and grads: those of run_sensitivities
    sens = deriv_param_all_times(sim, x, [obs])
    assert geo.values.shape == sens.values.shape and [g.shape for g in geo.grads] == [g.shape for g in sens.grads]
    assert float((geo.values - sens.values).abs().max()) <= NATIVE_RTOL * float(sens.values.abs().max())
    for got, want in zip(geo.grads, sens.grads):
        assert float(want.abs().max()) > 1e-3
        assert float((got - want).abs().max()) <= NATIVE_RTOL * float(want.abs().max())
    # without observables: empty values and grads of the Sensitivities shapes
    bare = sim.run_quantum_fisher(x)
    assert tuple(bare.values.shape) == (0, n_t) and [tuple(g.shape) for g in bare.grads] == [(0, n_t, 1), (0, n_t, 1), (0, n_t, 2)]
    assert torch.equal(bare.qfi, geo.qfi)


def test_public_route_with_a_state_overlap(cuda_device):
    """A StateOverlap yields two rows, Re and Im of c = <phi|psi>, whose grads are evolve_tangent's overlap rows."""
    sim, omega, area, coords = _basic_usage(cuda_device, evaluation_times=0.25)
    x = [omega, area, coords["q0"]]
    gen = torch.Generator().manual_seed(4242)
    target = _randn(gen, 16, cplx=True)
    target = target / target.norm()
    obs = DiagonalObservable(total_magnetization_diag(4))
    geo = sim.run_quantum_fisher(x, [obs, StateOverlap(target)], solver=SolverType.KRYLOV_SE)
    n_t = len(sim.evaluation_times)
    assert tuple(geo.values.shape) == (3, n_t) and [tuple(g.shape) for g in geo.grads] == [(3, n_t, 1), (3, n_t, 1), (3, n_t, 2)]
    ham = sim._hamiltonian
    d_amp, d_det, d_u = sim._table_tangents(x)
    psi0 = sim.initial_state
    psi_bd = psi0.reshape(psi0.shape[0], -1).transpose(0, 1).to(cuda_device)
    spec = ham.problem_spec(solver=SolverType.KRYLOV_SE, tol=S.tolerance_from_options({}), store_states=False)
    spec.overlaps = pack_overlaps([StateOverlap(target)], 16, 1, cuda_device)
    expect, dexpect = evolve_tangent(ham.amp_tables, ham.det_tables, ham.u_pairs, sim.evaluation_times.detach(), psi_bd, spec,
                                     obs.diag[None].to(cuda_device, torch.float64), d_amp=d_amp, d_det=d_det, d_u=d_u)
    assert tuple(dexpect.shape) == (4, 3, n_t, 1)
    assert float((geo.values - expect[:, :, 0]).abs().max()) <= NATIVE_RTOL * float(expect.abs().max())
    flat = torch.cat([g.reshape(3, n_t, -1) for g in geo.grads], dim=-1)  # (3, n_t, 4)
    want = dexpect[:, :, :, 0].permute(1, 2, 0).to(flat.device)
    for r in (1, 2):  # Re, Im of d c
        assert float(want[r].abs().max()) > 1e-3
        assert float((flat[r] - want[r]).abs().max()) <= NATIVE_RTOL * float(want[r].abs().max())
