"""Forward-mode (tangent) sweep on the GPU (rydiff_forward_tangent through pulser_diff_amd.solver.evolve_tangent and through
TorchEmulator.run_sensitivities).

1. Duality with the native adjoint: for seeded random directions (d_amp, d_det, d_u, d_psi0) and a seeded random cotangent w over
   (rows, n_t, B),   sum w * dexpect_d  ==  Re<g_amp, d_amp> + <g_det, d_det> + <g_u, d_u> + Re<g_psi0, d_psi0>   with the g_* of
   evolve(...).backward under w (torch's complex convention: g = dL/dRe + i dL/dIm, so the pairing is sum Re(conj(g) d)).
   Bar: 1e-9 relative to the larger side — one native gradient route against another (tests/test_gpu_sharded.py).
2. Values: expect_out of the tangent call against evolve's expect, 1e-10 (one native route against another, values).
3. Against the CPU oracle: d/ds of the dense map on terms0 + s * direction by reverse-mode autograd (shares nothing with the
   feature), all times, sum Z and an off-diagonal Pauli observable, 1e-8 relative to the largest entry (GRAD_RTOL of the Pauli tests).
4. The public route against the per-time deriv_param loop, 1e-9 relative to the largest entry.
Every problem comes from tests.helpers.random_terms(local=True, phase=True): several flip groups, complex coefficients, both
branches of the conjugation rule."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from oracle import restatement as R
from pulser_diff_amd import pulses as pl
from pulser_diff_amd.derivative import deriv_param, deriv_param_all_times
from pulser_diff_amd.observables import PauliObservable, pack_overlaps, StateOverlap
from pulser_diff_amd.solver import SolverType, evolve, evolve_tangent
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag
from tests.helpers import magnus_cf4_dense, random_terms, to_native

pytestmark = pytest.mark.gpu

DUALITY_RTOL = 1e-9
VALUE_ATOL = 1e-10
ORACLE_RTOL = 1e-8
PUBLIC_RTOL = 1e-9
N_SAMPLES, DT = 41, 0.004
TSAVE = (0.0, 0.0313, 0.0622, 0.0951, 0.1277, 0.1513)  # off the sample grid: DP5 stages mix two samples


def observable_set(n, seed=5):
    """The Pauli set of tests/test_gpu_pauli_observables.py, re-stated: sum X_j, sum Y_j, X_0 X_{N-1}, Z_1 Z_2, X_a Y_b Z_c and, from 13
    qubits, X_a X_b with distant flips plus a Z; weights seeded in [-1, 1]."""
    rng = np.random.default_rng(seed + n)
    w = lambda: float(rng.uniform(-1, 1))  # noqa: E731
    out = [PauliObservable(n, [(w(), {j: "X"}) for j in range(n)]), PauliObservable(n, [(w(), {j: "Y"}) for j in range(n)])]
    if n >= 2:
        out.append(PauliObservable(n, [(w(), {0: "X", n - 1: "X"})]))
    if n >= 3:
        out.append(PauliObservable(n, [(w(), {1: "Z", 2: "Z"})]))
        out.append(PauliObservable(n, [(w(), {n - 1: "X", 0: "Y", 1: "Z"})]))
    if n >= 13:
        out.append(PauliObservable(n, [(w(), {1: "X", n - 2: "X"}), (w(), {n - 1: "Z"})]))
    return out


def _randn(gen, *shape, cplx=False):
    return torch.randn(*shape, generator=gen, dtype=torch.complex128 if cplx else torch.float64)


# (n_qubits, solver, batch, coeff_batch, n_dir, which tangent inputs are given)
CASES = [
    (1, "KRYLOV_SE", 2, 1, 1, "adup"),    # one qubit: a block that is not full, no U
    (1, "DP5_SE", 2, 2, 3, "adup"),
    (3, "KRYLOV_SE", 2, 2, 3, "adup"),
    (3, "DP5_SE", 2, 1, 8, "adup"),
    (9, "KRYLOV_SE", 2, 1, 3, "adup"),    # two 256-thread blocks, partners across blocks
    (9, "DP5_SE", 2, 2, 1, "adup"),
    (13, "KRYLOV_SE", 2, 1, 3, "adup"),   # the adjoint side runs on another kernel family
    (13, "DP5_SE", 2, 2, 8, "adup"),
    (3, "KRYLOV_SE", 2, 1, 1, "a"),       # one case per single non-NULL tangent pointer
    (3, "DP5_SE", 2, 2, 3, "d"),
    (3, "DP5_SE", 2, 1, 1, "u"),
    (3, "KRYLOV_SE", 2, 1, 3, "p"),
]
_IDS = [f"N{n}-{s}-B{b}-cb{cb}-D{d}-{which}" for n, s, b, cb, d, which in CASES]


@lru_cache(maxsize=None)
def _duality_run(case):
    """One tangent sweep and one evolve + backward on the same problem; everything the duality and the value test compare."""
    n, solver_name, batch, cb, n_dir, which = case
    dev = torch.device("cuda:0")
    solver = SolverType[solver_name]
    terms = random_terms(n, N_SAMPLES, DT, seed=900 + n, local=True, phase=True)
    amp, det, u, spec = to_native(terms, dev, solver, store_states=False, batch_tables=cb)
    gen = torch.Generator().manual_seed(7000 + 31 * n + 7 * n_dir + cb)
    if cb > 1:  # per-trajectory tables really differ
        amp = amp * (1.0 + 0.1 * _randn(gen, cb, 1, 1).to(dev))
        det = det * (1.0 + 0.1 * _randn(gen, cb, 1, 1).to(dev))
    dim = 2**n
    psi0 = _randn(gen, batch, dim, cplx=True)
    psi0 = (psi0 / psi0.norm(dim=1, keepdim=True)).to(dev)
    target = _randn(gen, dim, batch if cb > 1 else 1, cplx=True)
    target = target / target.norm(dim=0, keepdim=True)
    spec.pauli = observable_set(n)
    spec.overlaps = pack_overlaps([StateOverlap(target)], dim, batch, dev)
    zdiag = total_magnetization_diag(n)[None].to(dev)
    tsave = torch.tensor(TSAVE, dtype=torch.float64)
    # directions, scaled like the inputs they perturb
    d_amp = (float(amp.abs().max()) * _randn(gen, n_dir, *amp.shape, cplx=True)).to(dev) if "a" in which else None
    d_det = (float(det.abs().max()) * _randn(gen, n_dir, *det.shape)).to(dev) if "d" in which else None
    d_u = (float(u.abs().max()) * _randn(gen, n_dir, *u.shape)).to(dev) if ("u" in which and u.numel()) else None
    d_psi = _randn(gen, n_dir, batch, dim, cplx=True).to(dev) / np.sqrt(dim) if "p" in which else None
    expect_t, dexpect = evolve_tangent(amp, det, u, tsave, psi0, spec, zdiag, d_amp=d_amp, d_det=d_det, d_u=d_u, d_psi0=d_psi)
    # the adjoint side
    leaves = [t.clone().requires_grad_(True) for t in (amp, det, u, psi0)]
    _, expect = evolve(leaves[0], leaves[1], leaves[2], tsave, leaves[3], spec, zdiag)
    w = _randn(gen, *expect.shape).to(dev)
    (w * expect).sum().backward()
    g_amp, g_det, g_u, g_psi = (t.grad for t in leaves)
    left, right, abs_terms = [], [], []
    for d in range(n_dir):
        prod = (w * dexpect[d]).double()
        left.append(float(prod.sum()))
        abs_terms.append(float(prod.abs().sum()))
        r = 0.0
        if d_amp is not None:
            r += float((g_amp.conj() * d_amp[d]).real.sum())
        if d_det is not None:
            r += float((g_det * d_det[d]).sum())
        if d_u is not None:
            r += float((g_u * d_u[d]).sum())
        if d_psi is not None:
            r += float((g_psi.conj() * d_psi[d]).real.sum())
        right.append(r)
    rows = 1 + len(spec.pauli) + 2
    assert tuple(dexpect.shape) == (n_dir, rows, len(TSAVE), batch) and tuple(expect_t.shape) == (rows, len(TSAVE), batch)
    assert not dexpect.requires_grad and not expect_t.requires_grad  # no autograd graph on the outputs
    return {"left": left, "right": right, "abs": abs_terms, "expect_tangent": expect_t.cpu().numpy(), "expect": expect.detach().cpu().numpy()}


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_tangent_sweep_is_dual_to_the_native_adjoint(case, cuda_device):
    run = _duality_run(case)
    for d, (lhs, rhs, abs_sum) in enumerate(zip(run["left"], run["right"], run["abs"])):
        big = max(abs(lhs), abs(rhs))
        print(f"direction {d}: tangent {lhs:+.15e}  adjoint {rhs:+.15e}  rel {abs(lhs - rhs) / big:.2e}  big / sum|terms| {big / abs_sum:.2e}")
        assert big > 1e-3 * abs_sum > 0.0  # cannot pass on zeros
        assert abs(lhs - rhs) <= DUALITY_RTOL * big


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_tangent_sweep_returns_the_values_of_evolve(case, cuda_device):
    run = _duality_run(case)
    err = float(np.abs(run["expect_tangent"] - run["expect"]).max())
    print(f"max |expect(tangent) - expect(evolve)| = {err:.2e}, max |expect| = {np.abs(run['expect']).max():.3f}")
    assert np.abs(run["expect"]).max() > 1e-2
    assert err <= VALUE_ATOL


def _shifted_terms(terms, d_amp, d_det, d_u, s):
    """terms + sum_j s[j] * direction_j as oracle HamTerms (tables in the order of amp_terms() / det_terms())."""
    amps = [c + sum(s[j] * d_amp[j][k] for j in range(len(s))) for k, (c, _) in enumerate(terms.amp_terms())]
    dets = [c + sum(s[j] * d_det[j][k] for j in range(len(s))) for k, (c, _) in enumerate(terms.det_terms())]
    u = terms.u_pairs + sum(s[j] * d_u[j] for j in range(len(s)))
    out = R.HamTerms(terms.n_qubits, u, amps[0], dets[0], terms.dt, terms.n_samples, terms.amp_targets, terms.det_targets)
    out.extra_amp = [(c, tg) for c, (_, tg) in zip(amps[1:], terms.extra_amp)]
    out.extra_det = [(c, tg) for c, (_, tg) in zip(dets[1:], terms.extra_det)]
    return out


@pytest.mark.parametrize("solver", [SolverType.KRYLOV_SE, SolverType.DP5_SE], ids=["KRYLOV_SE", "DP5_SE"])
@pytest.mark.parametrize("n", [4, 6])
def test_tangent_sweep_against_the_dense_oracle(n, solver, cuda_device):
    n_samples, dt, n_dir = 21, 0.005, 2
    terms = random_terms(n, n_samples, dt, seed=40 + n, local=True, phase=True)
    tsave = torch.tensor([0.0, 0.0213, 0.0488, 0.0911], dtype=torch.float64)
    gen = torch.Generator().manual_seed(77 + n)
    dim = 2**n
    psi0 = _randn(gen, dim, 1, cplx=True)
    psi0 = psi0 / psi0.norm()
    amp, det, u, spec = to_native(terms, cuda_device, solver)
    d_amp = 0.5 * _randn(gen, n_dir, *amp.shape[1:], cplx=True)
    d_det = 0.5 * _randn(gen, n_dir, *det.shape[1:])
    d_u = 0.5 * _randn(gen, n_dir, *u.shape)
    d_psi = _randn(gen, n_dir, dim, 1, cplx=True) / np.sqrt(dim)
    offdiag = PauliObservable(n, [(0.7, {0: "X", n - 1: "X"}), (-0.4, {1: "Y"})])
    zdiag = total_magnetization_diag(n)
    dense_o = offdiag.to_dense()

    def oracle(s):
        shifted = _shifted_terms(terms, d_amp, d_det, d_u, s)
        start = psi0 + sum(s[j] * d_psi[j] for j in range(n_dir))
        if solver == SolverType.KRYLOV_SE:
            states = R.krylov_map_dense(shifted, start, tsave)
        else:
            states = magnus_cf4_dense(shifted, start, tsave, h_max=2.5e-3 * (1e-9 / 1e-10) ** 0.25)  # the native default (tol 1e-9)
        return torch.stack([(states.abs() ** 2 * zdiag[None, :, None]).sum(1),
                            torch.einsum("tib,ij,tjb->tb", states.conj(), dense_o, states).real])  # (2, n_t, 1)

    ref = torch.autograd.functional.jacobian(oracle, torch.zeros(n_dir, dtype=torch.float64)).permute(3, 0, 1, 2).numpy()
    spec.pauli = [offdiag]
    _, dexpect = evolve_tangent(amp, det, u, tsave, psi0.T.contiguous().to(cuda_device), spec, zdiag[None].to(cuda_device),
                                d_amp=d_amp[:, None].to(cuda_device), d_det=d_det[:, None].to(cuda_device), d_u=d_u.to(cuda_device),
                                d_psi0=d_psi.permute(0, 2, 1).contiguous().to(cuda_device))
    got = dexpect.cpu().numpy()
    for d in range(n_dir):
        scale = np.abs(ref[d]).max()
        err = np.abs(got[d] - ref[d]).max()
        print(f"direction {d}: largest entry {scale:.3e}, max error {err:.3e} ({err / scale:.2e} relative)")
        assert scale > 1e-2
        assert err <= ORACLE_RTOL * scale


def _basic_usage(cuda_device, config=None, evaluation_times="Full", all_coords=False):
    """examples/basic_usage.py's sequence (4 atoms) with float64 parameters."""
    f64 = lambda v, grad: torch.tensor(v, dtype=torch.float64, requires_grad=grad)  # noqa: E731
    coords = {"q0": f64([0.0, 0.0], True), "q1": f64([0.0, 8.0], all_coords), "q2": f64([8.0, 0.0], all_coords),
              "q3": f64([8.0, 8.0], all_coords)}
    seq = pl.Sequence(pl.Register(coords), pl.MockDevice)
    seq.declare_channel("rydberg_global", "rydberg_global")
    omega, area = f64([5.0], True), f64([torch.pi], True)
    seq.add(pl.Pulse(pl.BlackmanWaveform(800, area), pl.RampWaveform(800, -5.0, 0.0), 0), "rydberg_global")
    seq.add(pl.Pulse.ConstantPulse(800, omega, 0.0, 0.0), "rydberg_global")
    sim = P.TorchEmulator.from_sequence(seq, sampling_rate=0.1, config=config, evaluation_times=evaluation_times,
                                        compute_device=cuda_device)
    return sim, omega, area, coords


def _loop(sim, x, obs, solver, dist_grad=False):
    """The per-time deriv_param loop of the reference's notebook; (n_t, ...) per tensor of x, and the values."""
    results = sim.run(dist_grad=dist_grad, solver=solver)
    f = results.expect([obs])[0].real
    times = sim.evaluation_times
    per_time = [deriv_param(f, x, times, float(times[k]) * 1000.0) for k in range(len(times))]
    return f.detach().cpu().numpy(), [torch.stack([g[i] for g in per_time]).detach().cpu().numpy() for i in range(len(x))]


def _compare(sens, values, grads):
    assert float(np.abs(sens.values[0].cpu().numpy() - values).max()) <= 1e-9 * 4
    for got, want in zip(sens.grads, grads):
        got = got[0].cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float64
        scale = np.abs(want).max()
        err = np.abs(got - want).max()
        print(f"shape {want.shape}: largest entry {scale:.3e}, max error {err:.3e} ({err / scale:.2e} relative)")
        assert scale > 1e-3
        assert err <= PUBLIC_RTOL * scale


def test_public_route_equals_the_per_time_loop(cuda_device):
    sim, omega, area, coords = _basic_usage(cuda_device)
    obs = DiagonalObservable(total_magnetization_diag(4))
    x = [omega, area, coords["q0"]]
    sens = deriv_param_all_times(sim, x, [obs])
    assert sens.route == "tangent"
    n_t = len(sim.evaluation_times)
    assert tuple(sens.values.shape) == (1, n_t) and [tuple(g.shape) for g in sens.grads] == [(1, n_t, 1), (1, n_t, 1), (1, n_t, 2)]
    _compare(sens, *_loop(sim, x, obs, SolverType.DP5_SE))


def test_public_route_with_a_distance(cuda_device):
    sim, omega, area, coords = _basic_usage(cuda_device, evaluation_times=0.25)
    obs = DiagonalObservable(total_magnetization_diag(4))
    sim.run(dist_grad=True, solver=SolverType.KRYLOV_SE)  # fills qq_distances
    x = [omega, sim.qq_distances["q1-q2"], sim.qq_distances["q0-q3"]]
    sens = deriv_param_all_times(sim, x, [obs], solver=SolverType.KRYLOV_SE, dist_grad=True)
    assert sens.route == "tangent"
    _compare(sens, *_loop(sim, x, obs, SolverType.KRYLOV_SE, dist_grad=True))


def test_public_route_chunks_ten_directions(cuda_device):
    sim, omega, area, coords = _basic_usage(cuda_device, evaluation_times=0.25, all_coords=True)
    obs = DiagonalObservable(total_magnetization_diag(4))
    x = [omega, area] + [coords[k] for k in ("q0", "q1", "q2", "q3")]  # 10 scalars: 8 + 2
    sens = deriv_param_all_times(sim, x, [obs], solver=SolverType.KRYLOV_SE)
    assert sens.route == "tangent"
    _compare(sens, *_loop(sim, x, obs, SolverType.KRYLOV_SE))


def test_public_route_falls_back_to_the_adjoint_loop_for_the_master_equation(cuda_device):
    sim, omega, area, coords = _basic_usage(cuda_device, config=P.SimConfig(noise="dephasing", dephasing_rate=0.5), evaluation_times=0.1)
    obs = DiagonalObservable(total_magnetization_diag(4))
    x = [omega, area, coords["q0"]]
    sens = deriv_param_all_times(sim, x, [obs])
    assert sens.route == "adjoint-loop"
    _compare(sens, *_loop(sim, x, obs, SolverType.DP5_SE))
