"""Occupation correlations on the GPU (RydProblem.bit_moments; csrc/moments_kernels.hpp): the rows S, B_q, B_qr and their gradients
through the C ABI (pulser_diff_amd.solver.evolve) and through the emulator.

  1  values and all five gradients against the dense oracle, N = 1 .. 10, both solvers, B = 2 with different unnormalised psi0;
     a random cotangent on every row, and one-hot cotangents on the S row, one single row and the first and last pair row
  2  past one tile (T = 12 tile bits): the same call is handed diagonal tables for S, two singles and four pairs; native rows
     against diagonal rows and the gradients of the two routes against each other, N = 11, 12, 13, 14, 17, 21; every tape mode at 13
  3  every block of the row layout in one call (tests/test_gpu_row_layout.py's problem, with the moments block behind the RDM block)
  4  zero-filled against NaN-filled workspaces (tests/test_gpu_workspace_contents.py), with the moments on
  5  two calls on the same input return bit-identical rows
  6  TorchEmulator.run(observables=[OccupationCorrelations()]) against the torch route on stored states, and against DiagonalObservable

Tolerances are the project's own; every use names its source line."""
import math

import numpy as np
import pytest
import torch

from oracle import restatement as R
from pulser_diff_amd.observables import OccupationCorrelations, moment_pair_row, moment_rows, occupation_moments
from pulser_diff_amd.solver import SolverType, evolve, split_moments, split_observables
from pulser_diff_amd.utils import DiagonalObservable
from tests.helpers import gershgorin_half_width, magnus_cf4_dense, random_terms, rel_err, tangent_rows_reference, to_native
from tests.test_gpu_pauli_observables import GRAD_RTOL, VALUE_ATOL  # :24, :23
from tests.test_gpu_rdm_observables import ROUTE_TOL  # :27
from tests.test_gpu_substepped_intervals import FAMILY_RTOL  # :53
from tests.test_gpu_tangent import PUBLIC_RTOL  # :34
from tests.test_gpu_workspace_contents import SAME_ROUTE_RTOL, TSAVE as WS_TSAVE, _both_fills, _compare, _problem as _ws_problem  # noqa: F401

pytestmark = pytest.mark.gpu

TILE_BITS = 12  # kMomTileBits


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


# ---- 1. the dense oracle --------------------------------------------------------------------------------------------------------
# 3 samples 45 ns apart, 4 save points off the sample grid, 64 ns in all: the gradients w.r.t. the detuning tables and the
# interactions are of third order in the run's length, and shorter runs leave them below the 1e-4 the checks ask of every reference
# gradient (sized with the CPU oracle: the smallest is 6e-4).  DP5_SE cuts the intervals at the one interior sample (45 ns): four
# pieces of at most 22.3 ns.  The run asks for tol = 1e-5, which puts the sub-step limit of the CF4 scheme at 44 ns (csrc/plan.hpp:
# 2.5 ns * (tol / 1e-10)^(1/4), shrinking like sqrt(128 / half width) beyond a half width of 128 rad/us): one CF4 step per piece in
# the oracle and in the library — asserted below, not assumed — so the dense reference stays at 8 exponentials at every size.  The
# reference is the same discrete map, so the agreement does not depend on tol.
O_SAMPLES, O_DT = 3, 0.045
O_TSAVE = (0.0, 0.0213, 0.0436, 0.0641)
O_DP5_TOL = 1e-5
O_DP5_H_MAX = 2.5e-3 * (O_DP5_TOL / 1e-10) ** 0.25
O_BATCH = 2
ORACLE_CASES = [(n, s) for n in (1, 2, 3, 6, 7, 9, 10) for s in ("KRYLOV_SE", "DP5_SE")]


def _one_hots(n, n_t, batch):
    """name -> cotangent (rows, n_t, B): the S row alone, one single row, the first and the last pair row, each at its own (k, b).
    (The S row sits at the first save point: <psi|psi> is conserved, so behind it only g_psi0 is not zero.)"""
    rows = moment_rows(n)
    out = {"S": torch.zeros(rows, n_t, batch, dtype=torch.float64), "single": torch.zeros(rows, n_t, batch, dtype=torch.float64)}
    out["S"][0, 0, 1] = 1.0
    out["single"][1 + n // 2, 1, 0] = 1.0
    if n >= 2:
        out["pairs"] = torch.zeros(rows, n_t, batch, dtype=torch.float64)
        out["pairs"][1 + n, 1, 1] = 1.0
        out["pairs"][rows - 1, 2, 0] += 1.0  # (2 qubits: the one pair row twice, at two save points)
    return out


@pytest.mark.parametrize("n,solver_name", ORACLE_CASES, ids=[f"N{n}-{s}" for n, s in ORACLE_CASES])
def test_values_and_gradients_match_the_dense_oracle(cuda_device, n, solver_name):
    """One wave (1 - 6 qubits), one workgroup (7 - 10) of the one-launch sweeps by the automatic kernel choice; the reference of a
    case is built once and serves the values, the random cotangent and the one-hot ones.  From 9 qubits on the time of a case is the
    CPU oracle's (autograd through 1024 x 1024 matrix exponentials), not the GPU's."""
    dev = cuda_device
    solver = SolverType[solver_name]
    terms = random_terms(n, O_SAMPLES, O_DT, seed=7300 + n, local=True, phase=True)
    tsave0 = torch.tensor(O_TSAVE, dtype=torch.float64)
    if solver == SolverType.DP5_SE:
        limit = O_DP5_H_MAX * math.sqrt(128.0 / max(gershgorin_half_width(terms), 128.0))
        cuts = sorted(set(O_TSAVE) | {O_DT})
        assert max(b - a for a, b in zip(cuts[:-1], cuts[1:])) < limit  # one CF4 step per piece on both sides
    gen = torch.Generator().manual_seed(9100 + n)
    psi0 = _randn(gen, 2 ** n, O_BATCH, cplx=True)
    psi0 = psi0 / psi0.norm(dim=0, keepdim=True) * torch.tensor([0.7, 1.4], dtype=torch.float64)  # norms != 1: the S row matters
    rows, n_t = moment_rows(n), len(O_TSAVE)
    cots = {"random": _randn(gen, rows, n_t, O_BATCH)}  # different on every row, save point and trajectory
    cots.update(_one_hots(n, n_t, O_BATCH))

    # the oracle: dense states, the rows by the torch route, autograd
    o_terms = R.HamTerms(n, terms.u_pairs.clone().requires_grad_(True), terms.amp_coeff.clone().requires_grad_(True),
                         terms.det_coeff.clone().requires_grad_(True), O_DT, O_SAMPLES, terms.amp_targets, terms.det_targets)
    o_terms.extra_amp = [(a.clone().requires_grad_(True), t) for a, t in terms.extra_amp]
    o_terms.extra_det = [(a.clone().requires_grad_(True), t) for a, t in terms.extra_det]
    o_ts, o_psi = tsave0.clone().requires_grad_(True), psi0.clone().requires_grad_(True)
    o_states = (R.krylov_map_dense(o_terms, o_psi, o_ts) if solver == SolverType.KRYLOV_SE
                else magnus_cf4_dense(o_terms, o_psi, o_ts, h_max=O_DP5_H_MAX))
    want = occupation_moments(o_states)
    o_amp_leaves, o_det_leaves = [a for a, _ in o_terms.amp_terms()], [a for a, _ in o_terms.det_terms()]
    o_leaves = o_amp_leaves + o_det_leaves + [o_ts, o_psi] + ([o_terms.u_pairs] if n > 1 else [])

    def oracle_grads(cot):
        g = torch.autograd.grad(want, o_leaves, grad_outputs=cot, retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(leaf) if x is None else x for x, leaf in zip(g, o_leaves)]
        ka, kd = len(o_amp_leaves), len(o_det_leaves)
        out = {"amp": torch.stack(g[:ka]), "det": torch.stack(g[ka:ka + kd]), "tsave": g[ka + kd], "psi0": g[ka + kd + 1]}
        if n > 1:
            out["u"] = g[ka + kd + 2]
        return {k: v.numpy() for k, v in out.items()}

    # native
    amp, det, u, spec = to_native(terms, dev, solver, tol=O_DP5_TOL if solver == SolverType.DP5_SE else 0.0, store_states=False)
    spec.moments = True
    leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(n > 1), tsave0.clone().requires_grad_(True),
              psi0.T.contiguous().to(dev).requires_grad_(True)]
    _, expect = evolve(*leaves, spec, None)
    assert tuple(expect.shape) == (rows, n_t, O_BATCH)
    got = expect.detach().cpu()
    val_err = float(((got - want.detach()).abs() / want.detach()[0]).max())
    print(f"MOMENTS N={n} {solver_name} {spec.options['_last_stats']['kernel_family']}: values, largest error / S {val_err:.2e}")
    assert val_err <= VALUE_ATOL  # tests/test_gpu_pauli_observables.py:23, relative to S

    def native_grads(cot):
        live = [t for t in leaves if t.requires_grad]
        g = dict(zip(("amp", "det", "u", "tsave", "psi0") if n > 1 else ("amp", "det", "tsave", "psi0"),
                     torch.autograd.grad(expect, live, grad_outputs=cot.to(dev), retain_graph=True)))
        g["amp"], g["det"], g["psi0"] = g["amp"].sum(0), g["det"].sum(0), g["psi0"].T
        return {k: v.cpu().numpy() for k, v in g.items()}

    scale_random = {}
    for name, cot in cots.items():
        g_want, g_got = oracle_grads(cot), native_grads(cot)
        assert g_want.keys() == g_got.keys() and len(g_got) == (5 if n > 1 else 4)
        for leaf in g_want:
            scale, err = float(np.abs(g_want[leaf]).max()), float(np.abs(g_got[leaf] - g_want[leaf]).max())
            print(f"MOMENTS N={n} {solver_name} cotangent {name}, g_{leaf}: largest entry {scale:.3e}, max error {err:.3e}")
            if name == "random":
                scale_random[leaf] = scale
                assert scale > 1e-4  # nothing passes on zeros
                assert err <= GRAD_RTOL * scale  # tests/test_gpu_pauli_observables.py:24
            else:
                # A one-hot gradient can be far smaller than the terms it is summed from, down to an exact zero (the S row: the norm
                # is conserved; a detuning gradient at short times), and the sweep's rounding error is set by the cotangent it
                # carries, not by the sum that cancels.  The unit cotangent is one term of the random one (entries of order one),
                # so the bar is the random cotangent's wherever the one-hot gradient is the smaller of the two.
                assert err <= GRAD_RTOL * max(scale, scale_random[leaf])  # tests/test_gpu_pauli_observables.py:24


# ---- 2. past one tile, against the diagonal-table route -------------------------------------------------------------------------
def _picked_bits(n):
    """Index bits of the S row, two singles (the lowest and the highest index bit) and four pairs: two lane bits (low-low), the
    highest bit with a lane bit (high-low past one tile), the two highest bits (high-high from 14 qubits on), a wave bit with one
    of a thread's own bits (low-low)."""
    return [(), (0,), (n - 1,), (0, 1), (3, n - 1), (n - 2, n - 1), (6, 9)]


def _moment_row_of(n, bits):
    qs = sorted(n - 1 - b for b in bits)
    return 0 if not qs else (1 + qs[0] if len(qs) == 1 else moment_pair_row(n, qs[0], qs[1]))


def _tables(n, dev):
    y = torch.arange(2 ** n, device=dev)
    out = []
    for bits in _picked_bits(n):
        t = torch.ones(2 ** n, dtype=torch.float64, device=dev)
        for b in bits:
            t = t * ((y >> b) & 1).to(torch.float64)
        out.append(t)
    return torch.stack(out)


def _route_case(n, dev, tape="auto", tape_steps=None):
    """-> (native rows picked, diagonal rows, gradients of the native-route loss, gradients of the diagonal-route loss) of ONE call
    that is handed both; the same random cotangent on both copies."""
    big = n >= 17
    batch, tsave0 = (1, (0.0, 0.0031, 0.0072)) if big else (2, (0.0, 0.0031, 0.0072, 0.0109))
    terms = random_terms(n, 10 if big else 13, 0.002, seed=7500 + n, local=True, phase=True)
    amp, det, u, spec = to_native(terms, dev, SolverType.KRYLOV_SE, store_states=False)
    spec.moments, spec.tape, spec.tape_steps = True, tape, tape_steps
    gen = torch.Generator().manual_seed(9500 + n)
    psi0 = _randn(gen, batch, 2 ** n, cplx=True)
    psi0 = (1.3 * psi0 / psi0.norm(dim=1, keepdim=True)).to(dev)
    leaves = [amp.requires_grad_(True), det.requires_grad_(True), u.requires_grad_(True),
              torch.tensor(tsave0, dtype=torch.float64, requires_grad=True), psi0.requires_grad_(True)]
    _, expect = evolve(*leaves, spec, _tables(n, dev))
    picked = _picked_bits(n)
    assert tuple(expect.shape) == (len(picked) + moment_rows(n), len(tsave0), batch)
    diag_rows, mom = split_moments(expect, n)
    native_rows = mom[[_moment_row_of(n, bits) for bits in picked]]
    w = _randn(gen, len(picked), len(tsave0), batch).to(dev)
    g_native = torch.autograd.grad((w * native_rows).sum(), leaves, retain_graph=True)
    g_diag = torch.autograd.grad((w * diag_rows).sum(), leaves)
    torch.cuda.synchronize()
    return native_rows.detach(), diag_rows.detach(), g_native, g_diag, spec.options["_last_stats"]


def _check_routes(label, native_rows, diag_rows, g_native, g_diag):
    val_err = float(((native_rows - diag_rows).abs() / diag_rows[0]).max())
    print(f"MOMENTS {label}: native rows against diagonal rows, largest difference / S {val_err:.2e}")
    assert val_err <= ROUTE_TOL  # tests/test_gpu_rdm_observables.py:27
    for name, a, b in zip(("amp", "det", "u", "tsave", "psi0"), g_native, g_diag):
        scale, err = float(b.abs().max()), rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(f"MOMENTS {label} g_{name}: largest entry {scale:.3e}, native route against diagonal route {err:.2e}")
        assert scale > 0.0
        assert err <= FAMILY_RTOL  # tests/test_gpu_substepped_intervals.py:53


@pytest.mark.parametrize("n", [TILE_BITS - 1, TILE_BITS, TILE_BITS + 1, TILE_BITS + 2, 17, 21])
def test_native_rows_equal_the_diagonal_route_past_one_tile(cuda_device, n):
    """A moments row is a diagonal observable with table y_q y_r, and that path is pinned to the oracle by the tests of the diagonal
    rows.  One tile (11, 12: the rows go straight out), 2 and 4 tiles (one high bit: no high-high pair yet; two), 32 tiles, and 21
    qubits: 512 tiles, eight trips of the second stage's loop over the tiles per row.  21 qubits run B = 1, 3 save points and 10
    samples: no dense reference is needed, and the case took 0.11 s on an MI355X."""
    native_rows, diag_rows, g_native, g_diag, stats = _route_case(n, cuda_device)
    _check_routes(f"N={n} {stats['kernel_family']} tape={stats['tape']}", native_rows, diag_rows, g_native, g_diag)


@pytest.mark.parametrize("tape,tape_steps", [("steps", None), ("full", None), ("partial", 1)])
def test_every_tape_mode_at_13_qubits(cuda_device, tape, tape_steps):
    """As tests/test_gpu_workspace_contents.py runs them: the cotangent kernel reads the state of a save point from wherever the
    tape mode keeps it."""
    native_rows, diag_rows, g_native, g_diag, stats = _route_case(13, cuda_device, tape, tape_steps)
    assert stats["tape"] == tape  # the mode asked for is the mode that ran
    _check_routes(f"N=13 tape={tape}", native_rows, diag_rows, g_native, g_diag)


# ---- 3. every block together --------------------------------------------------------------------------------------------------------
def test_every_block_of_the_row_layout_in_one_call(cuda_device):
    """The ket problem of tests/test_gpu_row_layout.py (4 qubits, B = 2, diagonal, Pauli, overlap, RDMs with m = 1 and 2) with the
    moments block behind the RDM block: the shape, the values of each block, and a one-hot gradient inside the moments block and
    inside the RDM block in front of it."""
    from tests.test_gpu_rdm_tangent import ORACLE_RTOL, VALUE_ATOL as ROW_VALUE_ATOL, _partial
    from tests.test_gpu_row_layout import BATCH, N, N_DIR, N_REAL, SUBSYSTEMS, _ket_call, _ket_rows, _ket_weights, _picked
    from tests.test_gpu_tangent_matrix import TSAVE_9, _problem, _terms_with_tables

    dev = cuda_device
    prob = _problem(N, BATCH, 1, N_DIR)
    diag, pauli, targets = _ket_rows(prob)
    tsave = torch.tensor(TSAVE_9, dtype=torch.float64)
    o_amp, o_det = prob["amp"][0].clone().requires_grad_(True), prob["det"][0].clone().requires_grad_(True)
    states = R.krylov_map_dense(_terms_with_tables(prob["terms"], o_amp, o_det), prob["psi0"].T.contiguous(), tsave)
    want_real = tangent_rows_reference(states, torch.zeros(len(tsave), 1, 2 ** N, BATCH, dtype=torch.complex128), diag, pauli, targets)[0]
    want_rdms = [_partial(states, states, qs, N) for qs in SUBSYSTEMS]
    want_mom = occupation_moments(states)
    spec, diag_dev = _ket_call(prob, dev)
    spec.moments = True
    amp, det = prob["amp"].to(dev).requires_grad_(True), prob["det"].to(dev).requires_grad_(True)
    _, expect = evolve(amp, det, prob["u"].to(dev), tsave, prob["psi0"].to(dev), spec, diag_dev)
    assert N_REAL == 6 and moment_rows(N) == 11
    assert tuple(expect.shape) == (6 + 8 + 32 + 11, len(tsave), BATCH)
    rest, got_mom = split_moments(expect, N)
    got_real, got_ov, got_rdms = split_observables(rest, 1, spec.rdms)
    got_real = torch.cat([got_real, got_ov.real, got_ov.imag])
    val_err = (got_real.detach().cpu() - want_real.detach()).abs().amax(dim=(1, 2)) / _ket_weights(prob)
    assert float(val_err.max()) <= ROW_VALUE_ATOL  # tests/test_gpu_row_layout.py:87
    for got, want in zip(got_rdms, want_rdms):
        assert float((got.detach().cpu() - want.detach()).abs().max()) <= ROW_VALUE_ATOL  # tests/test_gpu_row_layout.py:91
    mom_err = float(((got_mom.detach().cpu() - want_mom.detach()).abs() / want_mom.detach()[0]).max())
    print(f"MOMENTS every block: moments, largest error / S {mom_err:.2e}")
    assert mom_err <= VALUE_ATOL  # tests/test_gpu_pauli_observables.py:23, relative to S
    pair = moment_pair_row(N, 1, 3)
    got_picked = {"moments": got_mom[pair, 2, 1], "rdm": _picked(got_real, got_rdms)["rdm"]}
    want_picked = {"moments": want_mom[pair, 2, 1], "rdm": _picked(want_real, want_rdms)["rdm"]}
    for block in got_picked:
        g_amp, g_det = torch.autograd.grad(got_picked[block], [amp, det], retain_graph=True)
        w_amp, w_det = torch.autograd.grad(want_picked[block], [o_amp, o_det], retain_graph=True)
        for name, got, want in (("amp", g_amp[0].cpu(), w_amp), ("det", g_det[0].cpu(), w_det)):
            scale, err = float(want.abs().max()), float((got - want).abs().max())
            print(f"MOMENTS every block: gradient of the {block} row w.r.t. {name}: largest entry {scale:.3e}, max error {err:.3e}")
            assert scale > 1e-4  # nothing passes on zeros
            assert err <= ORACLE_RTOL * scale  # tests/test_gpu_row_layout.py:100


# ---- 4. workspace contents ------------------------------------------------------------------------------------------------------------
WS_CASES = [(n, s) for n in (3, 9, 13, TILE_BITS + 2) for s in ("KRYLOV_SE", "DP5_SE")]


@pytest.mark.parametrize("n,solver_name", WS_CASES, ids=[f"N{n}-{s}" for n, s in WS_CASES])
def test_moments_do_not_depend_on_workspace_contents(cuda_device, monkeypatch, n, solver_name):
    """The tile records of the first stage and the cotangent buffer are workspace regions: every entry that is read was written."""
    amp, det, u, spec, psi0, zdiag, gen = _ws_problem(n, solver_name, cuda_device)
    spec.moments = True
    tsave0 = torch.tensor(WS_TSAVE, dtype=torch.float64)
    rows = 1 + len(spec.pauli) + 2 + moment_rows(n)
    w = _randn(gen, rows, len(WS_TSAVE), psi0.shape[0]).to(cuda_device)

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (amp, det, u, tsave0, psi0)]
        _, expect = evolve(*leaves, spec, zdiag)
        (w * expect).sum().backward()
        out = {"expect": expect, "moments": split_moments(expect, n)[1], "g_amp": leaves[0].grad, "g_det": leaves[1].grad,
               "g_u": leaves[2].grad, "g_tsave": leaves[3].grad, "g_psi0": leaves[4].grad}
        return {k: (torch.view_as_real(v) if v.is_complex() else v).detach().cpu().numpy() for k, v in out.items()}

    zeros, nans = _both_fills(monkeypatch, run)
    _compare(f"MOMENTS N{n} {solver_name}", zeros, nans)  # finite, and within SAME_ROUTE_RTOL (tests/test_gpu_workspace_contents.py:33)


# ---- 5. bit-reproducibility -----------------------------------------------------------------------------------------------------------
def test_two_calls_return_bit_identical_rows(cuda_device):
    n = TILE_BITS + 2
    terms = random_terms(n, 13, 0.002, seed=7700, local=True, phase=True)
    amp, det, u, spec = to_native(terms, cuda_device, SolverType.KRYLOV_SE, store_states=True)
    spec.moments = True
    gen = torch.Generator().manual_seed(9700)
    psi0 = _randn(gen, 2, 2 ** n, cplx=True).to(cuda_device)
    tsave = torch.tensor((0.0, 0.0031, 0.0072, 0.0109), dtype=torch.float64)
    states_a, a = evolve(amp, det, u, tsave, psi0, spec, None)
    states_b, b = evolve(amp, det, u, tsave, psi0, spec, None)
    assert torch.equal(states_a, states_b)  # the input of the reduction is the same ...
    assert torch.equal(a, b)                # ... and so is every bit of the rows
    assert float(a[0].min()) > 0.0 and bool(torch.isfinite(a).all())


# ---- 6. the public path ---------------------------------------------------------------------------------------------------------------
def test_emulator_serves_occupations_correlations_and_the_structure_factor(cuda_device):
    from tests.test_gpu_tangent import _basic_usage

    signs = [1, -1, -1, 1]  # the Neel pattern of the 2 x 2 square (q0 (0,0), q1 (0,8), q2 (8,0), q3 (8,8))
    sim, omega, area, _ = _basic_usage(cuda_device)
    obs = OccupationCorrelations()
    native = sim.run(solver=SolverType.KRYLOV_SE, observables=[obs], store_states=False)
    with pytest.raises(RuntimeError, match="not stored"):
        native.states
    sim_b, omega_b, area_b, _ = _basic_usage(cuda_device)
    stored = sim_b.run(solver=SolverType.KRYLOV_SE, store_states=True)
    n_t = len(sim.evaluation_times)
    pairs = (("occupations", native.occupations(), stored.occupations(), (n_t, 4)),
             ("connected", native.occupation_correlations(connected=True), stored.occupation_correlations(connected=True), (n_t, 4, 4)),
             ("structure factor", native.structure_factor(signs), stored.structure_factor(signs), (n_t,)))
    for name, got, want, shape in pairs:
        assert tuple(got.shape) == tuple(want.shape) == shape
        scale, err = float(want.detach().abs().max()), float((got - want).detach().abs().max())
        print(f"MOMENTS public {name}: largest entry {scale:.3e}, native against stored states {err:.3e}")
        assert scale > 1e-3
        assert err <= PUBLIC_RTOL * scale  # tests/test_gpu_tangent.py:34
    # the gradient of the final structure factor reaches the pulse parameters
    g_native = torch.autograd.grad(native.structure_factor(signs)[-1], [omega, area])
    g_stored = torch.autograd.grad(stored.structure_factor(signs)[-1], [omega_b, area_b])
    for name, a, b in zip(("omega", "area"), g_native, g_stored):
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print(f"MOMENTS public d S(T) / d {name}: {float(a):+.9e} against {float(b):+.9e}")
        assert scale > 1e-4
        assert err <= GRAD_RTOL * scale  # tests/test_gpu_pauli_observables.py:24
    # <n_i> is the expectation of the projector on the level sample_state reports as "1": r, index value 0
    y = torch.arange(16)
    projectors = [DiagonalObservable(1.0 - ((y >> (3 - i)) & 1).to(torch.float64)) for i in range(4)]
    sim_c, _, _, _ = _basic_usage(cuda_device)
    diag = sim_c.run(solver=SolverType.KRYLOV_SE, observables=projectors, store_states=False)
    want = torch.stack([v.real for v in diag.expect(projectors)], dim=1)
    err = float((native.occupations().detach() - want.detach()).abs().max())
    print(f"MOMENTS public <n_i> against DiagonalObservable projectors: {err:.3e}")
    assert float(want.abs().max()) > 1e-3 and err <= PUBLIC_RTOL * float(want.abs().max())  # tests/test_gpu_tangent.py:34
