"""The native XY exchange term (RydProblem.xy_mode / xy_pairs / g_xy, csrc/xy_kernels.hpp) against the dense oracle up to 9 atoms and
against the matrix-free reference (tests/xy_exchange_reference.py) past it: states, every ket row, every gradient, through the
C ABI (solver.evolve) and through TorchEmulator.  Bars: 1e-9 for states and rows, 1e-8 for gradients relative to the largest entry."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import _native
from pulser_diff_amd import pulses as pl
from pulser_diff_amd import solver as S
from pulser_diff_amd.utils import DiagonalObservable
from pulser_diff_amd.solver import SolverType, evolve
from tests import xy_exchange_reference as X
from tests.helpers import SUBSTEP_RATIOS, gershgorin_half_width, product_state, random_terms, rel_err, substepped_tsave, to_native

pytestmark = pytest.mark.gpu

STATE_BAR, GRAD_BAR = 1e-9, 1e-8


def couplings(n: int, seed: int, scale: float = 3.0) -> torch.Tensor:
    """Mixed-sign J with one exact zero (where there are at least two pairs)."""
    g = torch.Generator().manual_seed(seed)
    J = scale * (2.0 * torch.rand(n * (n - 1) // 2, generator=g, dtype=torch.float64) - 1.0)
    if J.numel() >= 2:
        J[1] = 0.0
    return J


def problem(n: int, seed: int, local: bool = False, u_scale: float = 0.0):
    terms = random_terms(n, 25, 0.004, seed=seed, local=local)
    g = torch.Generator().manual_seed(seed + 1000)
    terms.u_pairs = u_scale * (2.0 * torch.rand(n * (n - 1) // 2, generator=g, dtype=torch.float64) - 1.0)
    return terms


def initial_states(n: int, batch: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.stack([product_state(n, g) for _ in range(batch)], dim=1)  # (dim, B)


def run_native(terms, J, mode, psi0, tsave, solver, dev, **spec_kw):
    amp, det, u, spec = to_native(terms, dev, solver)
    spec.xy_mode = mode
    for k, v in spec_kw.items():
        setattr(spec, k, v)
    states, expect = evolve(amp, det, u, tsave, psi0.T.contiguous().to(dev), spec, None, xy_pairs=J.to(dev))
    return states, expect, spec


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_small_registers_against_the_dense_oracle_and_the_dense_pair_route(cuda_device, n, mode):
    """N = 1 (no pair), 2 (dim 4 < one workgroup), 3, 5, 8 under KRYLOV_SE: a global drive with a phase, a detuning, mixed-sign J with
    an exact zero.  States against the dense oracle, and from 2 qubits on against the library's own dense pair terms."""
    terms = problem(n, 40 + n)
    J = couplings(n, 7 + n)
    psi0 = initial_states(n, 1, 3 + n)
    tsave = torch.linspace(0, 0.08, 5, dtype=torch.float64)
    states, _, spec = run_native(terms, J, mode, psi0, tsave, SolverType.KRYLOV_SE, cuda_device)
    assert spec.options["_last_stats"]["kernel_family"] == "direct"
    assert spec.options["_last_stats"]["kernel_fwd"] == "k_factor_xy"
    ref = X.dense_map(terms, J, mode, psi0, tsave, SolverType.KRYLOV_SE)
    got = states.cpu().permute(0, 2, 1).numpy()
    assert rel_err(got, ref.numpy()) < STATE_BAR
    if n >= 2:
        blocks = []
        for p, (a, b) in enumerate(itertools.combinations(range(n), 2)):
            blk = np.zeros((4, 4), dtype=np.complex128)
            blk[1, 2] = float(J[p])
            if mode == 1:
                blk[2, 1] = float(J[p])
            blocks.append((a, b, blk))
        amp, det, u, dspec = to_native(terms, cuda_device, SolverType.KRYLOV_SE)
        dspec.pair_terms = tuple(blocks)
        dense_states, _ = evolve(amp, det, u, tsave, psi0.T.contiguous().to(cuda_device), dspec, None)
        assert rel_err(got, dense_states.cpu().permute(0, 2, 1).numpy()) < STATE_BAR


# ---- 9 atoms: 36 pairs (more than RYDIFF_MAX_PAIR_TERMS), two workgroups -------------------------------------------------------------
N9 = 9
RDM_QUBITS = (2, 6)


def rows_reference(states: torch.Tensor, n: int, zdiag, pauli, phi) -> torch.Tensor:
    """The rows of `expect` in the library's order from states (n_t, dim, B): diagonal, Pauli, overlap Re / Im, RDM, moments."""
    n_t, dim, B = states.shape
    prob = states.abs() ** 2
    rows = [(prob * zdiag[None, :, None]).sum(1)]
    x = torch.arange(dim)
    acc = torch.zeros(n_t, B, dtype=torch.float64)
    for w, xq, zq in pauli:  # qubit masks: bit j = qubit j
        xm = sum(1 << (n - 1 - j) for j in range(n) if xq >> j & 1)
        zm = sum(1 << (n - 1 - j) for j in range(n) if zq >> j & 1)
        ny = bin(xq & zq).count("1")
        sign = torch.tensor([(-1.0) ** bin(int(v) & zm).count("1") for v in (x ^ xm)], dtype=torch.float64)
        applied = (1j ** ny) * sign[None, :, None] * states[:, x ^ xm, :]
        acc = acc + w * (states.conj() * applied).sum(1).real
    rows.append(acc)
    c = (phi.conj()[None, :, None] * states).sum(1)
    rows += [c.real, c.imag]
    t = states.reshape((n_t,) + (2,) * n + (B,))
    q1, q2 = RDM_QUBITS
    m = t.movedim((1 + q1, 1 + q2), (1, 2)).reshape(n_t, 4, -1, B)
    rho = torch.einsum("taeb,tceb->tacb", m, m.conj())
    for a in range(4):
        for a2 in range(4):
            rows += [rho[:, a, a2].real, rho[:, a, a2].imag]
    bits = [((x >> (n - 1 - q)) & 1).to(torch.float64) for q in range(n)]
    rows.append(prob.sum(1))
    rows += [(prob * bits[q][None, :, None]).sum(1) for q in range(n)]
    rows += [(prob * (bits[q] * bits[r])[None, :, None]).sum(1) for q, r in itertools.combinations(range(n), 2)]
    return torch.stack(rows)


def leaf_terms(terms):
    amp = terms.amp_coeff.clone().requires_grad_(True)
    det = terms.det_coeff.clone().requires_grad_(True)
    xa = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_amp]
    xd = [(c.clone().requires_grad_(True), tg) for c, tg in terms.extra_det]
    u = terms.u_pairs.clone().requires_grad_(True)
    return R.HamTerms(terms.n_qubits, u, amp, det, terms.dt, terms.n_samples, terms.amp_targets, terms.det_targets, xa, xd)


@pytest.mark.parametrize("mode,solver,u_scale", [(1, SolverType.KRYLOV_SE, 0.0), (2, SolverType.KRYLOV_SE, 0.0), (1, SolverType.DP5_SE, 0.0),
                                                 (2, SolverType.DP5_SE, 0.0), (1, SolverType.KRYLOV_SE, 2.0)])
def test_nine_atoms_states_rows_and_every_gradient(cuda_device, mode, solver, u_scale):
    """Both modes, a global and a local channel, both solvers; with u_scale != 0 a van der Waals term rides next to the exchange and
    g_u is checked next to g_xy.  The loss mixes the stored states and every kind of row."""
    n, dev = N9, cuda_device
    terms = problem(n, 90, local=True, u_scale=u_scale)
    J = couplings(n, 17, scale=2.0)
    psi0 = initial_states(n, 1, 5)
    n_t = 5 if solver == SolverType.KRYLOV_SE else 3
    tsave = torch.linspace(0.002, 0.002 + (0.015 if solver == SolverType.KRYLOV_SE else 0.007) * (n_t - 1), n_t, dtype=torch.float64)
    gen = torch.Generator().manual_seed(11)
    zdiag = R.total_magnetization_diag(n)
    pauli = [(0.7, 1 << 3, 1 << 5), (-0.4, (1 << 0) | (1 << 4), 1 << 4)]  # X_3 Z_5, X_0 Y_4
    phi = product_state(n, gen)
    first = np.array([0, 2], dtype=np.int32)
    px = np.array([t[1] for t in pauli], dtype=np.uint32)
    pz = np.array([t[2] for t in pauli], dtype=np.uint32)
    pw = np.array([t[0] for t in pauli], dtype=np.float64)

    # oracle
    ot = leaf_terms(terms)
    oJ = J.clone().requires_grad_(True)
    ots = tsave.clone().requires_grad_(True)
    opsi = psi0.clone().requires_grad_(True)
    ref = X.dense_map(ot, oJ, mode, opsi, ots, solver)
    ref_rows = rows_reference(ref, n, zdiag, pauli, phi)
    w_rows = torch.randn(ref_rows.shape, generator=gen, dtype=torch.float64)
    w_states = torch.randn(ref.shape, generator=gen, dtype=torch.float64) + 1j * torch.randn(ref.shape, generator=gen, dtype=torch.float64)
    (w_rows * ref_rows).sum().add((w_states.conj() * ref).sum().real).backward()

    # native
    amp, det, u, spec = to_native(terms, dev, solver)
    spec.xy_mode = mode
    spec.pauli = (first, px, pz, pw)
    spec.overlaps = phi[None, None, :].to(dev)
    spec.rdms = [sum(1 << q for q in RDM_QUBITS)]
    spec.moments = True
    amp.requires_grad_(True)
    det.requires_grad_(True)
    u.requires_grad_(True)
    Jd = J.to(dev).requires_grad_(True)
    ts = tsave.clone().requires_grad_(True)
    psi = psi0.T.contiguous().to(dev).requires_grad_(True)
    states, expect = evolve(amp, det, u, ts, psi, spec, zdiag[None].to(dev), xy_pairs=Jd)
    stats = spec.options["_last_stats"]
    assert stats["kernel_family"] == "direct" and stats["kernel_bwd"] == "k_factor_bwd_xy"
    if solver == SolverType.DP5_SE:  # (the reference's CF4 sub-step is the native default below that half width)
        assert 0.5 * (stats["spectral"][1] - stats["spectral"][0]) < 128.0
    got_states = states.detach().cpu().permute(0, 2, 1)
    assert rel_err(got_states.numpy(), ref.detach().numpy()) < STATE_BAR
    got_rows = expect.detach().cpu()
    assert got_rows.shape == ref_rows.shape
    scale = float(ref_rows.detach().abs().max())
    assert float((got_rows - ref_rows.detach()).abs().max()) < STATE_BAR * scale
    loss = (w_rows.to(dev) * expect).sum() + (w_states.permute(0, 2, 1).conj().to(dev) * states).sum().real
    loss.backward()
    torch.cuda.synchronize()
    amp_ref = torch.stack([ot.amp_coeff.grad] + [c.grad for c, _ in ot.extra_amp])
    det_ref = torch.stack([ot.det_coeff.grad] + [c.grad for c, _ in ot.extra_det])
    checks = {"g_amp": (amp.grad[0].cpu(), amp_ref), "g_det": (det.grad[0].cpu(), det_ref), "g_xy": (Jd.grad.cpu(), oJ.grad),
              "g_tsave": (ts.grad, ots.grad), "g_psi0": (psi.grad.cpu().T, opsi.grad)}
    if u_scale:
        checks["g_u"] = (u.grad.cpu(), ot.u_pairs.grad)
    errs = {k: rel_err(a.numpy(), b.numpy()) for k, (a, b) in checks.items()}
    print("xy n=9", mode, solver.name, u_scale, errs)
    assert max(errs.values()) < GRAD_BAR, errs
    assert float(oJ.grad[1]) != 0.0 and J[1] == 0.0  # the zero coupling still has a gradient


# ---- through TorchEmulator: 3 x 3 atoms in a magnetic field ------------------------------------------------------------------------
FIELD = (0.0, 1.0, 0.3)


def grid_coords(n_side: int = 3, spacing: float = 8.0, seed: int = 2) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor([[spacing * i, spacing * j] for i in range(n_side) for j in range(n_side)], dtype=torch.float64)
    return base + 0.4 * (2.0 * torch.rand(base.shape, generator=g, dtype=torch.float64) - 1.0)


def xy_sequence(coords, omega=3.0):
    seq = pl.Sequence(pl.Register.from_coordinates(coords), pl.MockDevice)
    seq.declare_channel("g", "mw_global")
    seq.set_magnetic_field(*FIELD)
    seq.add(pl.Pulse(pl.BlackmanWaveform(120, 2.1), pl.RampWaveform(120, -4.0, 3.0), 0.4), "g")
    seq.add(pl.Pulse.ConstantPulse(80, omega, 1.5, -0.2), "g")
    return seq


EVAL_TIMES = [0.04, 0.08, 0.12, 0.16, 0.2]


def emulator_oracle(seq, coords, hermitian: bool, freeze_angles: bool = False):
    """The oracle's dense generator from the sequence's raw per-ns samples (as tests/test_gpu_master_equation_sizes.py builds it),
    differentiable in `coords`; freeze_angles: the distances are leaves and the angular factor a constant (what dist_grad means)."""
    n = coords.shape[0]
    raw = pl.sample(seq).samples_list[0]
    zero = torch.zeros(1, dtype=torch.float64)
    n_full = raw.amp.numel() + 1
    c = 0.5 * torch.cat([raw.amp, zero]) * torch.exp(-1j * torch.cat([raw.phase, raw.phase[-1:]]).to(torch.complex128))
    d = -0.5 * torch.cat([raw.det, zero])
    c, d, dt, n_s = R.adapt_to_sampling_rate(c, 0.5, n_full), R.adapt_to_sampling_rate(d, 0.5, n_full), 0.002, int(0.5 * n_full)
    atoms = list(range(n))
    drive = R.reference_style_dense_H_t(coords.detach(), [(c, atoms)], [(d, atoms)], dt, n_s, "XY", magnetic_field=FIELD)
    idle = R.reference_style_dense_H_t(coords.detach(), [(torch.zeros_like(c), atoms)], [], dt, n_s, "XY", magnetic_field=FIELD)
    leaves = None
    if freeze_angles:
        J0 = X.couplings_from_dense(idle(0.0), n)
        r0 = torch.stack(R.pair_distances(coords.detach()))
        leaves = r0.clone().requires_grad_(True)
        Jt = J0 * r0**3 / leaves**3
        inter = X.exchange_dense(n, Jt, 2)
    else:
        inter = R.reference_style_dense_H_t(coords, [(torch.zeros_like(c), atoms)], [], dt, n_s, "XY", magnetic_field=FIELD)(0.0)
    inter = inter + inter.mH if hermitian else inter
    return (lambda t: drive(t) - idle(t) + inter), leaves


@pytest.mark.parametrize("hermitian", [False, True])
def test_emulator_nine_atoms_states_and_coordinate_gradient(cuda_device, hermitian):
    coords = grid_coords().requires_grad_(True)
    sim = P.TorchEmulator.from_sequence(xy_sequence(coords), sampling_rate=0.5, evaluation_times=EVAL_TIMES, xy_hermitian=hermitian)
    assert sim._hamiltonian.xy_mode == (1 if hermitian else 2) and not sim._hamiltonian.pair_terms
    res = sim.run(solver=SolverType.KRYLOV_SE)
    assert res.solver_stats["kernel_fwd"] == "k_factor_xy"
    ocoords = coords.detach().clone().requires_grad_(True)
    H_t, _ = emulator_oracle(xy_sequence(coords.detach()), ocoords, hermitian)
    psi0 = sim.initial_state.reshape(-1, 1).to(torch.complex128)
    ts = sim.evaluation_times.detach().cpu()
    ref = R.krylov_map_from_dense_H(H_t, psi0, ts)
    got = res.states.detach().cpu()
    assert rel_err(got.numpy(), ref.detach().numpy()) < STATE_BAR
    norms = (got.abs() ** 2).sum(1)
    if hermitian:
        assert float((norms - 1.0).abs().max()) < 1e-12
    else:
        assert abs(float(norms[-1, 0]) - 1.0) > 1e-3  # the literal generator is not Hermitian: the path is genuinely exercised
    w = torch.linspace(-1.0, 1.0, 2**9, dtype=torch.float64)
    f = res.expect([DiagonalObservable(w)])[0].real
    f[-1].backward()
    (ref[-1, :, 0].abs() ** 2 * w).sum().backward()
    assert rel_err(coords.grad.numpy(), ocoords.grad.numpy()) < GRAD_BAR


def test_emulator_dist_grad_reaches_the_distances_with_frozen_angles(cuda_device):
    coords = grid_coords()
    sim = P.TorchEmulator.from_sequence(xy_sequence(coords), sampling_rate=0.5, evaluation_times=EVAL_TIMES, xy_hermitian=True)
    res = sim.run(dist_grad=True, solver=SolverType.KRYLOV_SE)
    w = torch.linspace(-1.0, 1.0, 2**9, dtype=torch.float64)
    res.expect([DiagonalObservable(w)])[0].real[-1].backward()
    H_t, leaves = emulator_oracle(xy_sequence(coords), coords, True, freeze_angles=True)
    psi0 = sim.initial_state.reshape(-1, 1).to(torch.complex128)
    ref = R.krylov_map_from_dense_H(H_t, psi0, sim.evaluation_times.detach().cpu())
    (ref[-1, :, 0].abs() ** 2 * w).sum().backward()
    got = torch.stack([sim.dist_dict[k].grad for k in sim._hamiltonian._dist_dict])
    assert rel_err(got.numpy(), leaves.grad.numpy()) < GRAD_BAR


def test_emulator_eight_atoms_without_gradients_keeps_the_dense_route(cuda_device):
    coords = grid_coords()[:8]
    sim = P.TorchEmulator.from_sequence(xy_sequence(coords), sampling_rate=0.5, evaluation_times=EVAL_TIMES, xy_hermitian=True)
    spec = sim._hamiltonian.problem_spec()
    assert spec.xy_mode == 0 and len(spec.pair_terms) == 28
    forced = P.TorchEmulator.from_sequence(xy_sequence(coords), sampling_rate=0.5, evaluation_times=EVAL_TIMES, xy_hermitian=True,
                                           xy_native=True)
    assert forced._hamiltonian.problem_spec().xy_mode == 1
    a = sim.run(solver=SolverType.KRYLOV_SE).states.detach().cpu().numpy()
    b = forced.run(solver=SolverType.KRYLOV_SE).states.detach().cpu().numpy()
    assert rel_err(b, a) < STATE_BAR


def test_a_sensitivity_call_leaves_the_geometry_gradient_of_the_next_run_intact(cuda_device):
    """4 atoms whose coordinates carry a gradient: run_sensitivities borrows the dense pair terms (constants) for its own call; the
    run() after it is on the native exchange term again and delivers the same coords.grad as a run() on a new emulator."""
    w = torch.linspace(-1.0, 1.0, 2**4, dtype=torch.float64)
    grads = []
    for sensitivities_first in (True, False):
        coords = grid_coords()[:4].clone().requires_grad_(True)
        omega = torch.tensor(3.0, dtype=torch.float64, requires_grad=True)
        sim = P.TorchEmulator.from_sequence(xy_sequence(coords, omega), sampling_rate=0.5, evaluation_times=EVAL_TIMES, xy_hermitian=True)
        if sensitivities_first:
            sim.run_sensitivities([omega], [DiagonalObservable(w)], solver=SolverType.KRYLOV_SE)
        assert sim._hamiltonian.problem_spec().xy_mode == 1
        res = sim.run(solver=SolverType.KRYLOV_SE)
        assert res.solver_stats["kernel_fwd"] == "k_factor_xy"
        res.expect([DiagonalObservable(w)])[0].real[-1].backward()
        grads.append(coords.grad.clone())
    assert float(grads[1].abs().max()) > 0.0
    assert rel_err(grads[0].numpy(), grads[1].numpy()) < 1e-12


# ---- past the dense limit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [SolverType.KRYLOV_SE, SolverType.DP5_SE])
def test_thirteen_qubits_batched_against_the_matrix_free_reference(cuda_device, solver):
    """N = 13, B = 2, coeff_batch = 2 (the same tables twice: J is shared anyway), states and all gradients; a request for the full
    tape is downgraded to one state per save point."""
    n, dev, mode = 13, cuda_device, 1
    terms = random_terms(n, 25, 0.004, seed=130, local=True, amp_scale=3.0, det_scale=2.0)
    terms.u_pairs = torch.zeros_like(terms.u_pairs)
    J = couplings(n, 23, scale=1.0)
    psi0 = initial_states(n, 2, 9)
    n_t = 3
    tsave = torch.linspace(0.002, 0.002 + 0.006 * (n_t - 1), n_t, dtype=torch.float64)
    ot = leaf_terms(terms)
    oJ = J.clone().requires_grad_(True)
    opsi = psi0.clone().requires_grad_(True)
    ots = tsave.clone().requires_grad_(True)
    ref = X.matrix_free_map(ot, oJ, mode, opsi, ots, solver)
    gen = torch.Generator().manual_seed(4)
    w = torch.randn(ref.shape, generator=gen, dtype=torch.float64) + 1j * torch.randn(ref.shape, generator=gen, dtype=torch.float64)
    (w.conj() * ref).sum().real.backward()

    amp, det, u, spec = to_native(terms, dev, solver, batch_tables=2)
    spec.xy_mode = mode
    spec.tape = "full"
    spec.store_states = True
    amp.requires_grad_(True)
    det.requires_grad_(True)
    Jd = J.to(dev).requires_grad_(True)
    psi = psi0.T.contiguous().to(dev).requires_grad_(True)
    ts = tsave.clone().requires_grad_(True)
    states, _ = evolve(amp, det, u, ts, psi, spec, None, xy_pairs=Jd)
    stats = spec.options["_last_stats"]
    if solver == SolverType.DP5_SE:  # (the reference's CF4 sub-step is the native default below that half width)
        assert 0.5 * (stats["spectral"][1] - stats["spectral"][0]) < 128.0
    assert rel_err(states.detach().cpu().permute(0, 2, 1).numpy(), ref.detach().numpy()) < STATE_BAR
    (w.permute(0, 2, 1).conj().to(dev) * states).sum().real.backward()
    amp_ref = torch.stack([ot.amp_coeff.grad] + [c.grad for c, _ in ot.extra_amp])
    det_ref = torch.stack([ot.det_coeff.grad] + [c.grad for c, _ in ot.extra_det])
    errs = {"g_amp": rel_err(amp.grad.sum(0).cpu().numpy(), amp_ref.numpy()), "g_det": rel_err(det.grad.sum(0).cpu().numpy(), det_ref.numpy()),
            "g_xy": rel_err(Jd.grad.cpu().numpy(), oJ.grad.numpy()), "g_psi0": rel_err(psi.grad.cpu().T.numpy(), opsi.grad.numpy()),
            "g_tsave": rel_err(ts.grad.numpy(), ots.grad.numpy())}
    print("xy n=13", solver.name, errs)
    assert max(errs.values()) < GRAD_BAR, errs
    # need_tape = 2 is downgraded to 1, exactly as for pair terms
    pre = S._prepare(amp, det, u, tsave, psi, spec, None, xy_pairs=Jd)
    info = _native.RydPlanInfo()
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    _native.check(_native.lib().rydiff_plan(ctypes.byref(pre.call.problem), 2, 1, scratch.data_ptr(), None, ctypes.byref(info)))
    assert info.tape_mode == 1 and info.kernel_family == 2


def test_substepped_exponentials_at_nine_atoms(cuda_device):
    """Save intervals long enough for 1, 2, 1, 3, 2 sub-exponentials, built from the widened half-width (sum |J| on top of the
    tables' Gershgorin bound): states and g_xy."""
    n, dev, mode = N9, cuda_device, 1
    terms = random_terms(n, 25, 0.02, seed=91)  # (samples 20 ns apart: the whole run stays inside the tables)
    terms.u_pairs = torch.zeros_like(terms.u_pairs)
    J = couplings(n, 19)
    half = gershgorin_half_width(terms) + float(J.abs().sum())
    tsave = substepped_tsave(half, SUBSTEP_RATIOS["MIXED"])
    assert float(tsave[-1]) < terms.dt * (terms.n_samples - 2)
    psi0 = initial_states(n, 1, 6)
    oJ = J.clone().requires_grad_(True)
    ref = X.dense_map(terms, oJ, mode, psi0, tsave, SolverType.KRYLOV_SE)
    gen = torch.Generator().manual_seed(8)
    w = torch.randn(ref.shape, generator=gen, dtype=torch.float64) + 1j * torch.randn(ref.shape, generator=gen, dtype=torch.float64)
    (w.conj() * ref).sum().real.backward()
    amp, det, u, spec = to_native(terms, dev, SolverType.KRYLOV_SE)
    spec.xy_mode = mode
    Jd = J.to(dev).requires_grad_(True)
    states, _ = evolve(amp, det, u, tsave, psi0.T.contiguous().to(dev), spec, None, xy_pairs=Jd)
    st = spec.options["_last_stats"]
    assert st["total_factors"] == st["degree"] * (1 + 2 + 1 + 3 + 2), st
    assert rel_err(states.detach().cpu().permute(0, 2, 1).numpy(), ref.detach().numpy()) < STATE_BAR
    (w.permute(0, 2, 1).conj().to(dev) * states).sum().real.backward()
    assert rel_err(Jd.grad.cpu().numpy(), oJ.grad.numpy()) < GRAD_BAR


# ---- the C ABI itself: workspace contents, refusals -------------------------------------------------------------------------------
def raw_call(n, mode, dev, batch=1, with_J=True):
    terms = problem(n, 50 + n, local=n > 2)
    J = couplings(n, 29).to(dev)
    amp, det, u, spec = to_native(terms, dev, SolverType.KRYLOV_SE)
    spec.xy_mode = mode if mode in (0, 1, 2) else 1
    psi = initial_states(n, batch, 2).T.contiguous().to(dev)
    tsave = torch.linspace(0, 0.06, 4, dtype=torch.float64)
    pre = S._prepare(amp, det, u, tsave, psi, spec, None, xy_pairs=J if spec.xy_mode else None)
    pre.call.problem.xy_mode = mode
    if not with_J:
        pre.call.problem.xy_pairs = None
    return pre, J


def plan(pre, dev, need_tape=0, backward=0):
    info = _native.RydPlanInfo()
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    rc = _native.lib().rydiff_plan(ctypes.byref(pre.call.problem), need_tape, backward, scratch.data_ptr(), None, ctypes.byref(info))
    return rc, info


def test_backward_on_a_poisoned_workspace_overwrites_g_xy(cuda_device):
    """The same backward call twice, the workspace filled with NaN patterns in between: g_xy is overwritten and both runs agree to
    1e-13 relative (the atomics of the replicas may land in another order)."""
    dev, n = cuda_device, N9
    pre, J = raw_call(n, 1, dev)
    L = _native.lib()
    rc, info = plan(pre, dev, 0, 1)
    assert rc == 0, _native.last_error()
    p = pre.call.problem
    ws = torch.full((info.workspace_bytes // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
    states = torch.empty((pre.n_t, pre.batch, pre.dim), dtype=torch.complex128, device=dev)
    _native.check(L.rydiff_forward(ctypes.byref(p), ctypes.byref(info), pre.psi.data_ptr(), states.data_ptr(), None, ws.data_ptr(),
                                   ws.numel() * 8, 0, None))
    gen = torch.Generator().manual_seed(1)
    gs = torch.randn(states.shape, generator=gen, dtype=torch.float64).to(dev).to(torch.complex128)
    outs = []
    for fill in (float("nan"), -float("nan")):
        ws.fill_(fill)
        g_xy = torch.full_like(J, 1e300)
        p.g_xy = g_xy.data_ptr()
        _native.check(L.rydiff_backward(ctypes.byref(p), ctypes.byref(info), states.data_ptr(), gs.data_ptr(), None, None, None, None, None,
                                        None, ws.data_ptr(), ws.numel() * 8, 0, None))
        torch.cuda.synchronize()
        outs.append(g_xy.cpu())
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0.0
    assert float((outs[0] - outs[1]).abs().max()) <= 1e-13 * float(outs[0].abs().max())


def test_refusals_come_before_any_launch(cuda_device):
    dev, L = cuda_device, _native.lib()
    # RYDIFF_EINVAL
    for mode in (-1, 3):
        rc, _ = plan(raw_call(3, mode, dev)[0], dev)
        assert rc == _native.RYDIFF_EINVAL and "xy_mode" in _native.last_error()
    rc, _ = plan(raw_call(3, 1, dev, with_J=False)[0], dev)
    assert rc == _native.RYDIFF_EINVAL and "xy_pairs" in _native.last_error()
    rc, info1 = plan(raw_call(1, 1, dev, with_J=False)[0], dev)  # one qubit: no pair, no pointer needed
    assert rc == 0 and info1.kernel_family == 2
    # RYDIFF_ENOTIMPL
    def refused(mutate, word, n=4):
        pre, _ = raw_call(n, 1, dev)
        keep = mutate(pre.call.problem)
        rc, _ = plan(pre, dev)
        assert rc == _native.RYDIFF_ENOTIMPL and word in _native.last_error(), (rc, _native.last_error())
        return keep

    qubits = np.array([[0, 1]], dtype=np.uint32)
    table = np.zeros((1, 16), dtype=np.complex128)

    def pair_terms(p):
        p.n_pair_terms, p.pair_qubits, p.pair_tables = 1, qubits.ctypes.data, table.ctypes.data

    refused(pair_terms, "pair terms")
    refused(lambda p: setattr(p, "shard_bits", 1), "shard")
    refused(lambda p: (setattr(p, "dm_atoms", 2)), "density-matrix")
    refused(lambda p: setattr(p, "amp_conditioned_terms", 1), "conditioned")
    refused(lambda p: setattr(p, "det_ones_terms", 1), "ones-counting")
    refused(lambda p: setattr(p, "kernel_variant", 2), "kernel_variant")
    for variant in (0, 1, 9):
        pre, _ = raw_call(4, 2, dev)
        pre.call.problem.kernel_variant = variant
        rc, info = plan(pre, dev)
        assert rc == 0 and info.kernel_family == 2 and info.kernel_fwd == b"k_factor_xy"
    # the tangent, geometry and Fisher sweeps
    pre, _ = raw_call(4, 1, dev)
    rc, info = plan(pre, dev)
    assert rc == 0
    tg = _native.RydTangent()
    tg.n_dir = 1
    d_psi = torch.zeros((1, pre.batch, pre.dim), dtype=torch.complex128, device=dev)
    tg.d_psi0 = d_psi.data_ptr()
    p, pi, pt = ctypes.byref(pre.call.problem), ctypes.byref(info), ctypes.byref(tg)
    out = torch.zeros(64, dtype=torch.float64, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    assert L.rydiff_forward_tangent(p, pi, pt, pre.psi.data_ptr(), None, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == _native.RYDIFF_ENOTIMPL
    assert L.rydiff_forward_geometry(p, pi, pt, pre.psi.data_ptr(), None, None, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == _native.RYDIFF_ENOTIMPL
    assert L.rydiff_forward_fisher(p, pi, pt, pre.psi.data_ptr(), None, None, None, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == _native.RYDIFF_ENOTIMPL
    assert "XY exchange" in _native.last_error()
    terms = problem(4, 54, local=True)
    amp, det, u, spec = to_native(terms, dev, SolverType.KRYLOV_SE)
    spec.xy_mode = 1
    for fn in (S.evolve_tangent, S.evolve_geometry, S.evolve_fisher):
        with pytest.raises(NotImplementedError, match="XY exchange"):
            fn(amp, det, u, torch.linspace(0, 0.05, 3, dtype=torch.float64), pre.psi, spec, None, d_psi0=d_psi)
