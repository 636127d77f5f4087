"""Host side of the native XY exchange term: the couplings Hamiltonian.xy_pairs and their autograd against the oracle, the route
selection, the refusals that remain past 8 atoms, and the matrix-free reference (tests/xy_exchange_reference.py) pinned to the
dense oracle.  No GPU."""
from __future__ import annotations


import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import pulses as pl
from pulser_diff_amd.simconfig import SimConfig
from pulser_diff_amd.solver import SolverType
from pulser_diff_amd.utils import DiagonalObservable
from tests import xy_exchange_reference as X
from tests.helpers import random_terms, rel_err


def grid(n: int, seed: int = 2, spacing: float = 8.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor([[spacing * (k // 3), spacing * (k % 3)] for k in range(n)], dtype=torch.float64)
    return base + 0.4 * (2.0 * torch.rand(base.shape, generator=g, dtype=torch.float64) - 1.0)


def emulator(coords, field=(0.0, 1.0, 0.3), slm=None, config=None, **kw):
    seq = pl.Sequence(pl.Register.from_coordinates(coords), pl.MockDevice)
    if slm:
        seq.config_slm_mask(slm)
    seq.declare_channel("g", "mw_global")
    seq.set_magnetic_field(*field)
    seq.add(pl.Pulse.ConstantPulse(40, 3.0, 1.0, 0.2), "g")
    return P.TorchEmulator.from_sequence(seq, compute_device="cpu", config=config, **kw)


def oracle_couplings(coords: torch.Tensor, field) -> torch.Tensor:
    """Twice the oracle's U per pair, read off its literal dense interaction matrix (2 * int_mat)."""
    n = coords.shape[0]
    zero = torch.zeros(4, dtype=torch.complex128)
    H = R.reference_style_dense_H_t(coords, [(zero, list(range(n)))], [], 0.001, 4, "XY", magnetic_field=field)
    return X.couplings_from_dense(H(0.0), n)


@pytest.mark.parametrize("field", [(0.0, 1.0, 0.3), (0.0, 0.0, 30.0), (1.0, -2.0, 0.0)])
@pytest.mark.parametrize("n", [2, 5, 9])
def test_couplings_are_twice_the_oracles_u_and_their_autograd_matches(n, field):
    """Also a field that vanishes in the plane of the 2-D register (cos = 0 for every pair)."""
    coords = grid(n).requires_grad_(True)
    ham = emulator(coords, field, xy_hermitian=True)._hamiltonian
    ocoords = coords.detach().clone().requires_grad_(True)
    ref = oracle_couplings(ocoords, field)
    assert ham.xy_pairs.shape == (n * (n - 1) // 2,)
    assert rel_err(ham.xy_pairs.detach().numpy(), ref.detach().numpy()) < 1e-13
    w = torch.linspace(-1.0, 2.0, ref.numel(), dtype=torch.float64)
    (w * ham.xy_pairs).sum().backward()
    (w * ref).sum().backward()
    assert rel_err(coords.grad.numpy(), ocoords.grad.numpy()) < 1e-12


@pytest.mark.parametrize("n,grad,xy_native,route", [(8, False, None, "dense"), (8, True, None, "native"), (8, False, True, "native"),
                                                    (8, True, False, "dense"), (9, False, None, "native"), (9, False, True, "native"),
                                                    (3, False, None, "dense")])
@pytest.mark.parametrize("hermitian", [False, True])
def test_route_selection(n, grad, xy_native, route, hermitian):
    coords = grid(n).requires_grad_(grad)
    ham = emulator(coords, xy_hermitian=hermitian, xy_native=xy_native)._hamiltonian
    spec = ham.problem_spec()
    assert ham.xy_route() == route
    if route == "native":
        assert spec.xy_mode == (1 if hermitian else 2) and spec.pair_terms == ()
    else:
        assert spec.xy_mode == 0 and len(spec.pair_terms) == n * (n - 1) // 2


def test_nine_atoms_build_a_spec_and_an_explicit_matrix():
    """A 3 x 3 array used to raise NotImplementedError("The XY mode is limited to 8 qubits ...")."""
    coords = grid(9)
    sim = emulator(coords, xy_hermitian=True)
    spec = sim._hamiltonian.problem_spec(solver=SolverType.KRYLOV_SE)
    assert spec.n_qubits == 9 and spec.xy_mode == 1 and sim._hamiltonian.xy_pairs.numel() == 36
    h = sim.get_hamiltonian(10).to_dense()
    assert (h - h.mH).abs().max() < 1e-12
    xmat = X.exchange_dense(9, oracle_couplings(coords, (0.0, 1.0, 0.3)), 1)  # (double flips: no overlap with the drive's entries)
    assert float((h * (xmat != 0)).sub(xmat).abs().max()) < 1e-12


def test_the_native_and_the_dense_route_give_the_same_explicit_matrix():
    for hermitian in (False, True):
        a = emulator(grid(4), xy_hermitian=hermitian).get_hamiltonian(15).to_dense()
        b = emulator(grid(4), xy_hermitian=hermitian, xy_native=True).get_hamiltonian(15).to_dense()
        assert float((a - b).abs().max()) < 1e-14 * float(a.abs().max())  # (the couplings: torch arithmetic there, Python floats here)


def test_what_stays_on_the_dense_route_refuses_past_eight_atoms_by_name():
    coords = grid(9)
    with pytest.raises(NotImplementedError, match="limited to 8 qubits"):
        emulator(coords, xy_native=False)
    sim = emulator(coords, xy_hermitian=True)
    with pytest.raises(NotImplementedError, match=r"limited to 8 qubits for the master-equation solver \(DP5_ME\)"):
        sim.run(solver=SolverType.DP5_ME)
    obs = DiagonalObservable(torch.linspace(0.0, 1.0, 2**9, dtype=torch.float64))
    x = [torch.tensor(1.0, dtype=torch.float64, requires_grad=True)]
    with pytest.raises(NotImplementedError, match="limited to 8 qubits for run_sensitivities"):
        sim.run_sensitivities(x, [obs], solver=SolverType.KRYLOV_SE)
    with pytest.raises(NotImplementedError, match="limited to 8 qubits for run_rdm_sensitivities"):
        sim.run_rdm_sensitivities(x, [[0, 1]], solver=SolverType.KRYLOV_SE)
    with pytest.raises(NotImplementedError, match="limited to 8 qubits for run_occupation_sensitivities"):
        sim.run_occupation_sensitivities(x, solver=SolverType.KRYLOV_SE)
    with pytest.raises(NotImplementedError, match="limited to 8 qubits for run_quantum_fisher"):
        sim.run_quantum_fisher(x, solver=SolverType.KRYLOV_SE)
    with pytest.raises(NotImplementedError, match="limited to 8 qubits for run_classical_fisher"):
        sim.run_classical_fisher(x, solver=SolverType.KRYLOV_SE)
    noisy = emulator(coords, xy_hermitian=True, config=SimConfig(noise="SPAM", eta=0.4, runs=3))
    with pytest.raises(NotImplementedError, match="limited to 8 qubits for noisy runs that average over realisations"):
        noisy.run(solver=SolverType.KRYLOV_SE)
    with pytest.raises(NotImplementedError, match="dist_grad is not available in the XY mode for run_sensitivities"):
        emulator(grid(4), xy_hermitian=True).run_sensitivities(x, [DiagonalObservable(torch.ones(16, dtype=torch.float64))],
                                                               solver=SolverType.KRYLOV_SE, dist_grad=True)
    with pytest.raises(NotImplementedError, match="SLM mask"):
        emulator(grid(4), slm=["q0"])


def test_solver_entry_points_check_the_couplings_and_refuse_the_sweeps():
    from pulser_diff_amd import solver as S
    from tests.helpers import to_native

    terms = random_terms(3, 8, 0.004, seed=1)
    amp, det, u, spec = to_native(terms, "cpu", SolverType.KRYLOV_SE)
    spec.xy_mode = 1
    with pytest.raises(ValueError, match="xy_pairs"):
        S._check_shapes(spec, amp, det, u, None, 1)
    with pytest.raises(ValueError, match=r"N\(N-1\)/2 = 3"):
        S._check_shapes(spec, amp, det, u, None, 1, xy_pairs=torch.zeros(2, dtype=torch.float64))
    spec.xy_mode = 3
    with pytest.raises(ValueError, match="xy_mode"):
        S._check_shapes(spec, amp, det, u, None, 1, xy_pairs=torch.zeros(3, dtype=torch.float64))
    spec.xy_mode = 0
    with pytest.raises(ValueError, match="without ProblemSpec.xy_mode"):
        S._check_shapes(spec, amp, det, u, None, 1, xy_pairs=torch.zeros(3, dtype=torch.float64))
    spec.xy_mode = 2
    psi = torch.zeros(1, 8, dtype=torch.complex128)
    for fn in (S.evolve_tangent, S.evolve_geometry, S.evolve_fisher):
        with pytest.raises(NotImplementedError, match="XY exchange"):
            fn(amp, det, u, torch.linspace(0, 0.01, 2, dtype=torch.float64), psi, spec, None, d_psi0=psi[None])


@pytest.mark.parametrize("hermitian", [False, True])
@pytest.mark.parametrize("n", [3, 5, 8])
def test_matrix_free_reference_is_pinned_to_the_dense_oracle(n, hermitian):
    """States of the matrix-free reference against krylov_map_from_dense_H on the oracle's literal dense generator (plus the adjoint
    of its interaction-only part for the Hermitian form), the couplings taken from the coordinates; at 5 atoms its gradients — the
    hand-written backward of the exchange gathers — against autograd through the dense matrices, under both solvers."""
    field = (0.0, 1.0, 0.3)
    coords = grid(n)
    mode = 1 if hermitian else 2
    terms = random_terms(n, 25, 0.004, seed=20 + n, local=True)
    terms.u_pairs = torch.zeros_like(terms.u_pairs)
    J = oracle_couplings(coords, field)
    lit = R.reference_style_dense_H_t(coords, terms.amp_terms(), terms.det_terms(), terms.dt, terms.n_samples, "XY", magnetic_field=field)
    H_t = lit
    if hermitian:
        zero = [(torch.zeros_like(c), tg) for c, tg in terms.amp_terms()]
        idle = R.reference_style_dense_H_t(coords, zero, [], terms.dt, terms.n_samples, "XY", magnetic_field=field)
        H_t = lambda t: lit(t) + idle(t).mH  # noqa: E731
    g = torch.Generator().manual_seed(n)
    psi0 = torch.randn(2**n, 2, generator=g, dtype=torch.float64) + 1j * torch.randn(2**n, 2, generator=g, dtype=torch.float64)
    psi0 = psi0 / torch.linalg.norm(psi0, dim=0, keepdim=True)
    tsave = torch.linspace(0.0, 0.06, 4, dtype=torch.float64)
    ref = R.krylov_map_from_dense_H(H_t, psi0, tsave)
    got = X.matrix_free_map(terms, J, mode, psi0, tsave, SolverType.KRYLOV_SE)
    assert rel_err(got.numpy(), ref.numpy()) < 1e-12
    if n != 5:
        return
    for solver in (SolverType.KRYLOV_SE, SolverType.DP5_SE):
        grads = []
        for fn in (X.matrix_free_map, X.dense_map):
            Jl = J.clone().requires_grad_(True)
            pl_ = psi0.clone().requires_grad_(True)
            ts = tsave.clone().requires_grad_(True)
            out = fn(terms, Jl, mode, pl_, ts, solver)
            w = torch.linspace(-1.0, 1.0, out.numel(), dtype=torch.float64).reshape(out.shape)
            ((w * out.real).sum() + (w.flip(0) * out.imag).sum()).backward()
            grads.append((out.detach(), Jl.grad, pl_.grad, ts.grad))
        for a, b in zip(*grads):
            assert rel_err(a.numpy(), b.numpy()) < 1e-11


def test_a_call_that_borrows_the_dense_terms_leaves_the_native_route_in_place():
    """4 atoms on the native route (coordinates with a gradient; xy_native=True): the master-equation solver, an averaged noisy run
    and the sensitivity entry points switch to the dense pair terms for their own call only — here they end in the backend's
    refusal of a CPU device, after the switch — and the next problem_spec() is the native one again, couplings still attached to
    the coordinates."""
    coords = grid(4).requires_grad_(True)
    sim = emulator(coords, xy_hermitian=True)
    ham = sim._hamiltonian
    obs = DiagonalObservable(torch.linspace(0.0, 1.0, 16, dtype=torch.float64))
    x = [torch.tensor(1.0, dtype=torch.float64, requires_grad=True)]
    calls = [lambda: sim.run(solver=SolverType.DP5_ME), lambda: sim.run_sensitivities(x, [obs], solver=SolverType.KRYLOV_SE),
             lambda: sim.run_rdm_sensitivities(x, [[0, 1]], solver=SolverType.KRYLOV_SE),
             lambda: sim.run_occupation_sensitivities(x, solver=SolverType.KRYLOV_SE)]
    for call in calls:
        seen = []
        original = ham.require_dense_xy
        ham.require_dense_xy = lambda what, o=original: (o(what), seen.append((ham.xy_mode, len(ham.pair_terms))))[0]
        try:
            with pytest.raises(Exception):
                call()
        finally:
            del ham.require_dense_xy
        assert seen == [(0, 6)]  # the call did run on the dense terms ...
        spec = ham.problem_spec()
        assert ham.xy_route() == "native" and spec.xy_mode == 1 and spec.pair_terms == ()  # ... and gave the route back
        assert ham.xy_pairs.requires_grad
    forced = emulator(grid(4), xy_hermitian=True, xy_native=True)
    with pytest.raises(Exception):
        forced.run(solver=SolverType.DP5_ME)
    assert forced._hamiltonian.problem_spec().xy_mode == 1


def test_dist_grad_is_refused_where_the_run_stays_on_the_dense_route():
    """run(dist_grad=True) on the master equation (asked for, or forced by collapse noise) and on averaged noisy runs used to raise in
    the XY mode and still does: the dense blocks are constants, and no distance becomes a leaf."""
    sim = emulator(grid(4), xy_hermitian=True)
    with pytest.raises(NotImplementedError, match=r"dist_grad is not available in the XY mode for the master-equation solver \(DP5_ME\)"):
        sim.run(dist_grad=True, solver=SolverType.DP5_ME)
    noisy = emulator(grid(4), xy_hermitian=True, config=SimConfig(noise="SPAM", eta=0.4, runs=3))
    with pytest.raises(NotImplementedError, match="dist_grad is not available in the XY mode for noisy runs that average"):
        noisy.run(dist_grad=True, solver=SolverType.KRYLOV_SE)
    for s_ in (sim, noisy):
        assert s_.dist_dict == {} and s_._hamiltonian.xy_mode == 0 and not s_._hamiltonian._xy_dist_grad


def test_a_refresh_puts_the_angular_factor_back_into_the_graph():
    """dist_grad freezes the angular factor of J; after refresh_from_sequence the distances are functions of the coordinates again,
    and so must the angles be: the gradient of the couplings equals that of a new emulator."""
    def sequence(c):
        seq = pl.Sequence(pl.Register.from_coordinates(c), pl.MockDevice)
        seq.declare_channel("g", "mw_global")
        seq.set_magnetic_field(0.0, 1.0, 0.3)
        seq.add(pl.Pulse.ConstantPulse(40, 3.0, 1.0, 0.2), "g")
        return seq

    sim = emulator(grid(5), xy_hermitian=True)
    sim._enable_dist_grad()
    assert sim._hamiltonian._xy_dist_grad and sim._hamiltonian.xy_mode == 1
    c1 = grid(5, seed=7).requires_grad_(True)
    assert sim.refresh_from_sequence(sequence(c1))
    c2 = c1.detach().clone().requires_grad_(True)
    new = emulator(c2, xy_hermitian=True)
    w = torch.linspace(-1.0, 2.0, 10, dtype=torch.float64)
    (w * sim._hamiltonian.xy_pairs).sum().backward()
    (w * new._hamiltonian.xy_pairs).sum().backward()
    assert rel_err(c1.grad.numpy(), c2.grad.numpy()) < 1e-13
