"""Tangent sweep with the native XY exchange (RYDIFF_TANGENT_XY, k_factor_tangent<D, false, true>: the stencil of xy_kernels.hpp over the
state and all D tangent states, couplings with tangents d_xy of their own) against tests/xy_tangent_reference.py — the dense
forward-mode reference, no autograd — entry by entry, at the bars of tests/test_gpu_tangent_matrix.py: dexpect within
ORACLE_RTOL = 1e-8 of each direction's largest reference entry, values within VALUE_ATOL = 1e-9 of the row's weight, every non-zero
direction's largest reference entry above 1e-2, a zero direction exactly zero.  Rows: one diagonal row, observable_set(n), one
StateOverlap; B = 2.  Couplings and terms: the generators of tests/test_gpu_xy_exchange.py (mixed-sign J with an exact zero, a global
and a local channel, a van der Waals term next to the exchange).

Shapes (the kernel walks row i of the stencil in chunks of TangentChunk<D> = 8 / 4 / 2 pairs for D = 1 / 2..3 / 4..8):
  N = 2 (one pair, 4 amplitudes), N = 3, N = 5 at D = 4, 5, 8 (chunks of 2 against rows of 4, 3, 2, 1; 5 is padded to 6), both
  modes and both solvers; N = 9 at D = 1 (row 0 fills one chunk of 8 exactly; two workgroups); N = 10 at D = 1, 2, 3, 6 (row 0
  spills into a second chunk; four workgroups; past the 8 atoms of the dense route).  Direction cases at N = 3: only d_xy, no d_xy,
  per-trajectory tables, 13 directions (a chunk of 8 and a padded chunk of 5).  Direction 1 of every problem is zero.
Further: duality with the native reverse sweep's g_xy at 12 atoms (DUALITY_RTOL), the Gram matrices of the geometry / Fisher sweeps at
4 atoms, and the emulator on a 3 x 3 grid with xy_native=True (PUBLIC_RTOL against the adjoint loop).

Measured on an MI355X: tangents at most 1.9e-12 of the direction's largest entry, values 2.2e-13 of the row weight (bars 1e-8 and 1e-9);
gram 7.3e-14 (mode 1) and 2.2e-13 (mode 2) against 1e-8; the emulator's sweep within 6e-15 of the adjoint loop, relative.  Reference
CPU time: 4.5 to 5 s per 10-qubit problem (shared by its cases), 1.4 s at 9 qubits, below a second up to 5.

Every test here fails without the feature: the parent's sweeps answer xy_mode != 0 with RYDIFF_ENOTIMPL / NotImplementedError."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import pulses as pl
from pulser_diff_amd.geometry import classical_fisher_information, quantum_fisher_information
from pulser_diff_amd.hamiltonian import Hamiltonian
from pulser_diff_amd.observables import StateOverlap, pack_overlaps
from pulser_diff_amd.solver import SolverType, evolve, evolve_fisher, evolve_geometry, evolve_tangent
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.helpers import tangent_rows_reference, to_native
from tests.test_gpu_classical_fisher import _psd_bar
from tests.test_gpu_tangent import DUALITY_RTOL, ORACLE_RTOL, PUBLIC_RTOL, _randn, observable_set
from tests.test_gpu_tangent_matrix import TSAVE, _terms_with_tables
from tests.test_gpu_tangent_pair_terms import TSAVE as TSAVE_SHORT
from tests.test_gpu_xy_exchange import couplings, initial_states, problem
from tests.xy_tangent_reference import xy_tangent_reference

pytestmark = pytest.mark.gpu

VALUE_ATOL = 1e-9
BATCH = 2


def _tsave(n, solver_name):
    """Four save points over the whole sequence up to 5 atoms; at 9 and 10 the short tuples of tests/test_gpu_tangent_pair_terms.py."""
    return TSAVE if n <= 5 else TSAVE_SHORT[solver_name]


@lru_cache(maxsize=None)
def _problem(n, mode, solver_name, n_dir, cb=1):
    """One seeded problem on the CPU with every tangent input for n_dir directions, direction 1 zero: computed once, never modified."""
    terms = problem(n, 300 + n, local=True, u_scale=1.0)
    amp, det, u, _ = to_native(terms, "cpu", SolverType.KRYLOV_SE, batch_tables=cb)
    gen = torch.Generator().manual_seed(73000 + 101 * n + 7 * mode + cb)
    if cb > 1:
        amp = amp * (1.0 + 0.1 * _randn(gen, cb, 1, 1))
        det = det * (1.0 + 0.1 * _randn(gen, cb, 1, 1))
    J = couplings(n, 40 + n)
    dim = 2 ** n
    psi0 = initial_states(n, BATCH, 9 + n).T.contiguous()  # (B, dim)
    scale = 8.0 if solver_name == "KRYLOV_SE" else 1.0  # (tests/test_gpu_tangent_matrix.py: KRYLOV_SE reads the tables once per interval)
    d = {"a": scale * float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True),
         "d": scale * float(det.abs().max()) * _randn(gen, n_dir, *det.shape),
         "u": _randn(gen, n_dir, u.numel()),
         "x": 3.0 * _randn(gen, n_dir, J.numel()),  # the size of the couplings
         "p": _randn(gen, n_dir, BATCH, dim, cplx=True) / np.sqrt(dim)}
    if n_dir > 1:
        for t in d.values():
            t[1] = 0.0
    target = psi0.T + 0.5 * _randn(gen, dim, BATCH, cplx=True) / np.sqrt(dim)
    target = target / target.norm(dim=0, keepdim=True)
    ref_terms = [_terms_with_tables(terms, amp[b], det[b]) for b in range(BATCH)] if cb > 1 else terms
    return dict(n=n, mode=mode, terms=terms, ref_terms=ref_terms, amp=amp, det=det, u=u, J=J, psi0=psi0, d=d, target=target,
                tsave=torch.tensor(_tsave(n, solver_name), dtype=torch.float64), solver=solver_name, cb=cb)


def _pick(prob, which, flag, n_dir):
    return prob["d"][flag][:n_dir] if flag in which else None


@lru_cache(maxsize=None)
def _reference(n, mode, solver_name, n_dir, which="adupx", cb=1):
    """Dense states (n_t, dim, B) and tangent states (n_t, n_dir, dim, B): built once per problem, sliced by the cases."""
    prob = _problem(n, mode, solver_name, n_dir, cb)
    d_amp, d_det = _pick(prob, which, "a", n_dir), _pick(prob, which, "d", n_dir)
    if cb == 1:  # shared tables: (n_dir, K, n)
        d_amp = None if d_amp is None else d_amp[:, 0]
        d_det = None if d_det is None else d_det[:, 0]
    d_psi = _pick(prob, which, "p", n_dir)
    return xy_tangent_reference(prob["ref_terms"], prob["J"], mode, d_amp, d_det, _pick(prob, which, "u", n_dir),
                                _pick(prob, which, "x", n_dir), prob["psi0"].T.contiguous(),
                                None if d_psi is None else d_psi.permute(0, 2, 1).contiguous(), prob["tsave"], SolverType[solver_name])


def _native_inputs(prob, dev, store_states=False):
    _, _, _, spec = to_native(prob["terms"], dev, SolverType[prob["solver"]], store_states=store_states)
    spec.xy_mode = prob["mode"]
    args = (prob["amp"].to(dev), prob["det"].to(dev), prob["u"].to(dev), prob["tsave"], prob["psi0"].to(dev), spec)
    return args, spec


def _tangent_kw(prob, which, n_dir, dev):
    names = {"a": "d_amp", "d": "d_det", "u": "d_u", "p": "d_psi0", "x": "d_xy"}
    return {names[f]: prob["d"][f][:n_dir].to(dev) for f in which}


def _check(case_id, prob, ref, which, n_dir, dev):
    """evolve_tangent on directions 0:n_dir against the reference, entry by entry."""
    n = prob["n"]
    dim = 2 ** n
    args, spec = _native_inputs(prob, dev)
    pauli = observable_set(n)
    spec.pauli = pauli
    spec.overlaps = pack_overlaps([StateOverlap(prob["target"])], dim, BATCH, dev)
    diag = total_magnetization_diag(n)[None]
    expect, dexpect = evolve_tangent(*args, diag.to(dev), xy_pairs=prob["J"].to(dev), **_tangent_kw(prob, which, n_dir, dev))
    states, tangents = ref
    want_val, want_der = tangent_rows_reference(states, tangents[:, :n_dir], diag, pauli, [prob["target"]])
    got_val, got_der = expect.cpu(), dexpect.cpu()
    assert tuple(got_der.shape) == tuple(want_der.shape) and tuple(got_val.shape) == tuple(want_val.shape)
    assert bool(torch.isfinite(got_der).all()) and bool(torch.isfinite(got_val).all())
    weights = torch.tensor([float(diag.abs().max())] + [sum(abs(w) for w, _, _ in p.terms) for p in pauli] + [1.0, 1.0], dtype=torch.float64)
    val_err = float(((got_val - want_val).abs().amax(dim=(1, 2)) / weights).max())
    print(f"{case_id}: values, largest error / row weight {val_err:.2e}")
    for d in range(n_dir):
        scale = float(want_der[d].abs().max())
        err = float((got_der[d] - want_der[d]).abs().max())
        print(f"{case_id}: direction {d}: largest entry {scale:.3e}, max error {err:.3e}")
        if d == 1:  # the zero direction stays exactly zero
            assert float(got_der[d].abs().max()) == 0.0 and scale == 0.0
        else:
            assert scale > 1e-2  # nothing passes on zeros
            assert err <= ORACLE_RTOL * scale
    assert float(want_val.abs().max()) > 1e-2
    assert val_err <= VALUE_ATOL


# ---- small registers: both modes, both solvers -------------------------------------------------------------------------------------
SMALL = [(2, 2), (3, 3), (5, 4), (5, 5), (5, 8)]


@pytest.mark.parametrize("solver_name", ["KRYLOV_SE", "DP5_SE"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,n_dir", SMALL, ids=[f"N{n}-D{d}" for n, d in SMALL])
def test_small_registers_match_the_dense_reference(cuda_device, n, n_dir, mode, solver_name):
    n_max = 8 if n == 5 else n_dir
    prob = _problem(n, mode, solver_name, n_max)
    _check(f"XY N={n} mode {mode} {solver_name} D={n_dir}", prob, _reference(n, mode, solver_name, n_max), "adupx", n_dir, cuda_device)


# ---- 9 and 10 atoms: more than one workgroup, rows of the stencil against the chunk of 8 ---------------------------------------------
LARGE = [(9, 1, 1, "KRYLOV_SE"), (9, 1, 2, "DP5_SE"), (10, 1, 1, "KRYLOV_SE"), (10, 2, 1, "KRYLOV_SE"), (10, 3, 1, "KRYLOV_SE"),
         (10, 6, 1, "KRYLOV_SE"), (10, 6, 2, "DP5_SE")]


@pytest.mark.parametrize("n,n_dir,mode,solver_name", LARGE, ids=[f"N{n}-D{d}-mode{m}-{s}" for n, d, m, s in LARGE])
def test_nine_and_ten_atoms_match_the_dense_reference(cuda_device, n, n_dir, mode, solver_name):
    n_max = 1 if n == 9 else 6
    prob = _problem(n, mode, solver_name, n_max)
    _check(f"XY N={n} mode {mode} {solver_name} D={n_dir}", prob, _reference(n, mode, solver_name, n_max), "adupx", n_dir, cuda_device)


# ---- direction cases at 3 atoms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("which", ["x", "adup"], ids=["only-d_xy", "no-d_xy"])
def test_single_kinds_of_tangent_inputs(cuda_device, which, mode):
    prob = _problem(3, mode, "KRYLOV_SE", 3)
    _check(f"XY N=3 mode {mode} {which}", prob, _reference(3, mode, "KRYLOV_SE", 3, which), which, 3, cuda_device)


def test_per_trajectory_tables(cuda_device):
    prob = _problem(3, 1, "KRYLOV_SE", 3, cb=2)
    _check("XY N=3 per-trajectory tables", prob, _reference(3, 1, "KRYLOV_SE", 3, "adupx", 2), "adupx", 3, cuda_device)


@pytest.mark.parametrize("mode", [1, 2])
def test_thirteen_directions_run_in_a_chunk_of_eight_and_a_padded_chunk_of_five(cuda_device, mode):
    prob = _problem(3, mode, "DP5_SE", 13)
    _check(f"XY N=3 mode {mode} 13 directions", prob, _reference(3, mode, "DP5_SE", 13), "adupx", 13, cuda_device)


# ---- duality with the reverse sweep at 12 atoms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,solver_name", [(1, "KRYLOV_SE"), (2, "DP5_SE")])
def test_duality_with_the_native_exchange_gradient_at_twelve_atoms(cuda_device, mode, solver_name):
    """Past any dense reference: dexpect of a d_xy-only direction is sum_p dJ_p g_xy[p] of evolve(...).backward() with a one-hot
    cotangent on the same row, time and trajectory."""
    n, dev = 12, cuda_device
    prob = _problem(n, mode, solver_name, 1)
    args, spec = _native_inputs(prob, dev)
    spec.pauli = observable_set(n)
    spec.overlaps = pack_overlaps([StateOverlap(prob["target"])], 2 ** n, BATCH, dev)
    diag = total_magnetization_diag(n)[None].to(dev)
    dJ = prob["d"]["x"][:1].to(dev)
    _, dexpect = evolve_tangent(*args, diag, xy_pairs=prob["J"].to(dev), d_xy=dJ)
    Jd = prob["J"].to(dev).requires_grad_(True)
    _, expect = evolve(*args, diag, xy_pairs=Jd)
    rows, n_t = expect.shape[0], expect.shape[1]
    scale = float(dexpect.abs().max())
    assert scale > 1e-2
    picks = [(0, n_t - 1, 0), (1, 1, 1), (3, n_t - 1, 1), (rows - 2, 1, 0), (rows - 1, n_t - 1, 1)]  # diagonal, Pauli, overlap Re / Im
    for r, k, b in picks:
        cot = torch.zeros_like(expect)
        cot[r, k, b] = 1.0
        (g_xy,) = torch.autograd.grad(expect, Jd, grad_outputs=cot, retain_graph=True)
        want = float((g_xy * dJ[0]).sum())
        got = float(dexpect[0, r, k, b])
        print(f"duality N=12 mode {mode} {solver_name} row {r} k {k} b {b}: tangent {got:.6e}, adjoint {want:.6e}, scale {scale:.2e}")
        assert abs(got - want) <= DUALITY_RTOL * scale


# ---- geometry and Fisher at 4 atoms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_gram_matrices_at_four_atoms(cuda_device, mode):
    n, n_dir, dev = 4, 3, cuda_device
    prob = _problem(n, mode, "KRYLOV_SE", n_dir)
    states, tangents = _reference(n, mode, "KRYLOV_SE", n_dir)
    args, _ = _native_inputs(prob, dev)
    kw = dict(xy_pairs=prob["J"].to(dev), **_tangent_kw(prob, "adupx", n_dir, dev))
    _, _, gram, cgram = evolve_fisher(*args, None, **kw)
    _, _, gram2, cgram2 = evolve_fisher(*args, None, **kw)
    _, _, gram3 = evolve_geometry(*args, None, **kw)
    assert torch.equal(gram, gram2) and torch.equal(cgram, cgram2) and torch.equal(gram, gram3)
    vecs = torch.cat([states[:, None], tangents], dim=1)  # (n_t, 1 + D, dim, B)
    want = torch.einsum("tixb,tjxb->tbij", vecs.conj(), vecs)
    err = float((gram.cpu() - want).abs().max() / want.abs().max())
    print(f"XY N=4 mode {mode}: gram against the reference tangents' inner products {err:.2e}")
    assert err <= 1e-8
    if mode == 1:  # a Hermitian generator: F_C <= F_Q as matrices, up to the rounding of the classical Gram matrix
        gap = (quantum_fisher_information(gram) - classical_fisher_information(cgram)).cpu()
        lam = torch.linalg.eigvalsh(0.5 * (gap + gap.transpose(-1, -2))).min(dim=-1).values
        bar = _psd_bar(gram.cpu(), 2 ** n)
        print(f"XY N=4: smallest eigenvalue of F_Q - F_C {float(lam.min()):.3e}, smallest bar {-float(bar.max()):.3e}")
        assert bool((lam >= -bar).all())


# ---- the emulator on a 3 x 3 grid -------------------------------------------------------------------------------------------------
def _grid_emulator(dev, monkeypatch):
    monkeypatch.setattr(Hamiltonian, "_warned_xy", True)
    gen = torch.Generator().manual_seed(4)
    coords = torch.tensor([[8.0 * (k // 3), 8.0 * (k % 3)] for k in range(9)], dtype=torch.float64)
    coords = (coords + 0.4 * (2.0 * torch.rand(coords.shape, generator=gen, dtype=torch.float64) - 1.0)).requires_grad_(True)
    omega = torch.tensor(3.0, dtype=torch.float64, requires_grad=True)
    seq = pl.Sequence(pl.Register.from_coordinates(coords), pl.MockDevice)
    seq.declare_channel("g", "mw_global")
    seq.set_magnetic_field(0.0, 1.0, 0.3)
    seq.add(pl.Pulse.ConstantPulse(200, omega, 1.0, 0.2), "g")
    sim = P.TorchEmulator.from_sequence(seq, sampling_rate=0.2, evaluation_times=[0.0, 0.05, 0.1, 0.15, 0.2], compute_device=dev,
                                        xy_hermitian=True, xy_native=True)
    return sim, omega, coords


def test_emulator_with_the_native_exchange_on_a_three_by_three_grid(cuda_device, monkeypatch):
    sim, omega, coords = _grid_emulator(cuda_device, monkeypatch)
    assert len(sim.evaluation_times) == 5
    x = [omega, coords]
    obs = [DiagonalObservable(total_magnetization_diag(9)), observable_set(9)[2]]
    tan = sim.run_sensitivities(x, obs, solver=SolverType.KRYLOV_SE)
    assert tan.route == "tangent"
    loop = sim.run_sensitivities(x, obs, solver=SolverType.KRYLOV_SE, route="adjoint-loop")
    assert loop.route == "adjoint-loop"
    assert float((tan.values.cpu() - loop.values.cpu()).abs().max()) <= 4e-9
    for got, want, name in zip(tan.grads, loop.grads, ("omega", "coordinates")):
        got, want = got.cpu(), want.cpu()
        assert got.shape == want.shape
        for o in range(2):  # relative to the observable's largest derivative w.r.t. this tensor over all times
            scale = float(want[o].abs().max())
            err = float((got[o] - want[o]).abs().max())
            print(f"3x3 XY grid, observable {o}, d/d{name}: largest entry {scale:.3e}, max error {err:.3e}")
            assert scale > 1e-4
            assert err <= PUBLIC_RTOL * scale
    occ = sim.run_occupation_sensitivities(x, solver=SolverType.KRYLOV_SE)
    qfi = sim.run_quantum_fisher(x, solver=SolverType.KRYLOV_SE)
    d_occ = occ.dmoments[1]  # (rows, n_t, B, 9, 2): w.r.t. the coordinates
    assert tuple(d_occ.shape[-2:]) == (9, 2) and bool(torch.isfinite(d_occ).all())
    assert float(d_occ[1:].abs().amax(dim=(0, 1, 2)).min()) > 0.0  # every coordinate moves some occupation moment
    f = qfi.qfi  # (n_t, D, D) with D = 1 + 18
    assert tuple(f.shape[-2:]) == (19, 19) and bool(torch.isfinite(f).all())
    coord_block = f[1:, 1:, 1:]
    assert float(torch.diagonal(coord_block, dim1=-2, dim2=-1).abs().min()) > 0.0  # every coordinate moves the state
    spec = sim._hamiltonian.problem_spec()
    assert spec.xy_mode == 1 and spec.pair_terms == () and sim._hamiltonian.xy_route() == "native"
