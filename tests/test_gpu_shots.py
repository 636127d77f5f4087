"""Native measurement shots on the GPU (RydProblem.n_shots / shot_*, pulser_diff_amd.shots): the sampling rule is deterministic
given the uniforms, so every check is an exact or a bracketed comparison — nothing here is statistical.

Kernel families covered (RydPlanInfo.kernel_family / kernel_fwd are asserted, so a case cannot silently run elsewhere): the one-wave
lane sweep (3, 6 qubits), the one-workgroup persistent sweep (9, 11), the direct kernels (13, variant 1), the chained tile passes
(13, 14, variant 2) and the blocks of two factors (14, variant 17); 1 and 3 trajectories; both solvers at 9 and 13 qubits.  Sizes
around the 2^10-amplitude chunk of the sampling kernels: below one chunk (3, 6, 9), two chunks (11), 8 and 16 chunks (13, 14).

The bracket of the evolved-state checks: with C_ref the longdouble cumulative sum of |states_out|^2 of the same call, shot x of
uniform u must satisfy  C_ref[x-1] - d <= u*S <= C_ref[x] + d  and p[x] > 0,  d = 2^(N-50) * S: eight times the worst-case bound
(2^N - 1) * 2^-53 * S on any summation order of 2^N non-negative doubles.  Derived, not measured.

Gradients with and without shots run the same kernels on the same data; they may differ by the order of atomic accumulation only,
bar 1e-10 relative to the largest entry (the suite's bar between two native routes, tests/test_gpu_overlap_observables.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pulser_diff_amd as P
from pulser_diff_amd import _native
from pulser_diff_amd import pulses as pl
from pulser_diff_amd.shots import SHOT_NONE, ShotRequest, indices_to_bitstrings, sample_indices_reference
from pulser_diff_amd.simresults import CoherentResults, NoisyResults
from pulser_diff_amd.solver import SolverType, _Call, evolve
from tests.helpers import random_terms, to_native

pytestmark = pytest.mark.gpu

ONE_BELOW = 1.0 - 2.0 ** -53
ROUTE_TOL = 1e-10
N_TSAVE = 4

# (qubits, kernel_variant, kernel family the plan must report, substring of kernel_fwd)
FAMILIES = [(3, 0, "lanes", "k_lanes_fwd"), (6, 0, "lanes", "k_lanes_fwd"), (9, 0, "persistent", "k_persist"),
            (11, 0, "persistent", "k_persist"), (13, 1, "direct", "k_factor_direct"), (13, 2, "chained-tiles", "k_chain<"),
            (14, 2, "chained-tiles", "k_chain<"), (14, 17, "chained-tiles", "k_chain2<")]
CASES = [(n, v, fam, kern, b, SolverType.KRYLOV_SE) for n, v, fam, kern in FAMILIES for b in (1, 3)]
CASES += [(9, 0, "persistent", "k_persist", 1, SolverType.DP5_SE), (13, 1, "direct", "k_factor_direct", 1, SolverType.DP5_SE)]
IDS = [f"N{n}-v{v}-B{b}-{s.name}" for n, v, _, _, b, s in CASES]


def _problem(n, variant, solver, device, store_states=True):
    """A short run (three save intervals, 9 samples).  Variant 17 (blocks of two factors) takes one phase-free global drive."""
    simple = variant == 17
    terms = random_terms(n, 9, 0.002, seed=900 + n, local=not simple, phase=not simple)
    amp, det, u, spec = to_native(terms, device, solver, store_states=store_states)
    spec.kernel_variant = variant
    if simple:
        amp = amp.real.contiguous()
    return amp, det, u, spec, torch.linspace(0, 0.012, N_TSAVE, dtype=torch.float64)


def _run(n, variant, solver, device, psi_bd, request, store_states=True, family=None, kernel=None):
    amp, det, u, spec, tsave = _problem(n, variant, solver, device, store_states)
    spec.shots = request
    states, _ = evolve(amp, det, u, tsave, psi_bd.to(device), spec, None)
    torch.cuda.synchronize()
    stats = spec.options["_last_stats"]
    if family is not None:
        assert stats["kernel_family"] == family and kernel in stats["kernel_fwd"], stats
    assert request.indices.shape == (len(request.time_indices), psi_bd.shape[0], request.n_shots) and request.indices.dtype == torch.int64
    return states, request.indices.cpu().numpy()


def _exact_js(n, seed):
    dim = 2 ** n
    js = {0, dim - 1}
    for m in range(0, dim + 1, 1024):
        js.update(j for j in (m - 1, m, m + 1) if 0 <= j < dim)
    js = sorted(js) + np.random.default_rng(seed).integers(0, dim, size=200).tolist()
    return np.asarray(js, dtype=np.int64)


@pytest.mark.parametrize("n,variant,family,kernel,batch,solver", CASES, ids=IDS)
def test_exact_on_the_start_state(cuda_device, n, variant, family, kernel, batch, solver):
    """psi0 = all ones: p = 1, S = 2^N, every partial sum is an exact integer in any order; u = j / 2^N must return x = j."""
    dim = 2 ** n
    js = np.stack([_exact_js(n, 10 * n + b) for b in range(batch)])                 # (B, shots): other random j per trajectory
    uniforms = torch.from_numpy(js.astype(np.float64) / dim)[None]                  # (1, B, shots)
    request = ShotRequest(js.shape[1], times=[0], uniforms=uniforms)
    _, got = _run(n, variant, solver, cuda_device, torch.ones(batch, dim, dtype=torch.complex128), request, family=family, kernel=kernel)
    assert request.time_indices == (0,)
    wrong = np.flatnonzero((got[0] != js).reshape(-1))
    assert wrong.size == 0, (got[0].reshape(-1)[wrong[:8]], js.reshape(-1)[wrong[:8]])


@pytest.mark.parametrize("n,variant,family,kernel,batch,solver", CASES, ids=IDS)
def test_one_hot_and_sparse_states(cuda_device, n, variant, family, kernel, batch, solver):
    """|g...g> (the last index): every uniform returns it.  A state on five scattered indices (the first and the last among them) with
    dyadic amplitudes, p = 1/2, 1/4, 1/8, 1/16, 1/16 (S = 1): sums and u * S (u on a 2^-20 grid, 0 and 1 - 2^-53) are exact in
    float64 as in longdouble, so the result must equal the host reference bit for bit and never sit on an empty amplitude."""
    dim = 2 ** n
    g = np.random.default_rng(77 + n)
    grid = g.integers(0, 2 ** 20, size=(batch, 300)).astype(np.float64) / 2 ** 20
    edge = np.tile(np.array([0.0, ONE_BELOW, 0.5, 0.75, 0.875, 0.9375, float("nan"), -1.0, 2.0]), (batch, 1))
    uniforms = torch.from_numpy(np.concatenate([edge, grid], axis=1))[None]
    ground = torch.zeros(batch, dim, dtype=torch.complex128)
    ground[:, dim - 1] = 1.0
    request = ShotRequest(uniforms.shape[2], times=[0], uniforms=uniforms)
    _, got = _run(n, variant, solver, cuda_device, ground, request, family=family, kernel=kernel)
    assert (got == dim - 1).all()

    amps = [0.5 + 0.5j, 0.5, 0.25 + 0.25j, 0.25, -0.25j]
    sparse = torch.zeros(batch, dim, dtype=torch.complex128)
    for b in range(batch):
        where = np.concatenate([[0, dim - 1], g.choice(np.arange(1, dim - 1), size=3, replace=False)])
        for a, x in zip(np.roll(amps, b), where):
            sparse[b, int(x)] = complex(a)
    probs = (sparse.real ** 2 + sparse.imag ** 2).numpy()
    assert (probs.sum(1) == 1.0).all()
    request = ShotRequest(uniforms.shape[2], times=[0], uniforms=uniforms)
    _, got = _run(n, variant, solver, cuda_device, sparse, request)
    assert (np.take_along_axis(probs, got[0], axis=1) > 0).all()
    want = sample_indices_reference(probs, uniforms[0].numpy())
    assert (got[0] == want).all(), np.argwhere(got[0] != want)[:8]
    assert set(np.unique(got[0][0]).tolist()) == set(np.flatnonzero(probs[0]).tolist())  # (every populated index is reachable)


def _random_psi0(n, batch):
    psi0 = torch.randn(batch, 2 ** n, generator=torch.Generator().manual_seed(40 + n), dtype=torch.complex128)
    return psi0 / psi0.norm(dim=1, keepdim=True)


def _uniforms(n, batch, n_times):
    u = torch.rand(n_times, batch, 256, generator=torch.Generator().manual_seed(3 * n + batch), dtype=torch.float64)
    u[:, :, 0] = 0.0
    u[:, :, 1] = ONE_BELOW
    return u


def _check_bracket(n, states, uniforms, got):
    """Every shot of every sampled time and trajectory against the longdouble cumulative sum of |states|^2; no shot is excluded."""
    st = states.cpu().numpy()
    worst = 0.0
    for k in range(st.shape[0]):
        for b in range(st.shape[1]):
            p = st[k, b].real ** 2 + st[k, b].imag ** 2
            cum = np.concatenate([[np.longdouble(0)], np.cumsum(p.astype(np.longdouble))])
            total = cum[-1]
            delta = np.longdouble(2.0 ** (n - 50)) * total
            x = got[k, b]
            assert (x != SHOT_NONE).all() and (x >= 0).all() and (x < p.size).all()
            tau = uniforms[k, b].numpy().astype(np.longdouble) * total
            lo, hi = cum[x] - delta, cum[x + 1] + delta
            miss = max(float((lo - tau).max()), float((tau - hi).max())) / float(total)
            worst = max(worst, miss)
            assert (lo <= tau).all() and (tau <= hi).all() and (p[x] > 0).all(), (k, b, miss)
    return worst


@pytest.fixture(scope="module")
def evolved(cuda_device):
    """Run 3 of every case, computed once: stored states, uniforms and shots at every save point."""
    cache = {}

    def get(n, variant, family, kernel, batch, solver):
        key = (n, variant, batch, solver)
        if key not in cache:
            uniforms = _uniforms(n, batch, N_TSAVE)
            request = ShotRequest(uniforms.shape[2], times="all", uniforms=uniforms)
            states, got = _run(n, variant, solver, cuda_device, _random_psi0(n, batch), request, family=family, kernel=kernel)
            assert request.time_indices == tuple(range(N_TSAVE))
            cache[key] = (states, uniforms, got)
        return cache[key]

    return get


@pytest.mark.parametrize("n,variant,family,kernel,batch,solver", CASES, ids=IDS)
def test_bracket_on_evolved_states(cuda_device, evolved, n, variant, family, kernel, batch, solver):
    states, uniforms, got = evolved(n, variant, family, kernel, batch, solver)
    assert states.shape == (N_TSAVE, batch, 2 ** n)
    worst = _check_bracket(n, states, uniforms, got)
    print(f"N={n} variant {variant} B={batch} {solver.name}: worst excess over the exact bracket {max(worst, 0.0):.3e} * S (bar {2.0 ** (n - 50):.3e})")
    # u = 0 returns the first populated amplitude, u = 1 - 2^-53 one whose cumulative value is S within the bar (a dense random state)
    assert (got[:, :, 0] == 0).all() and (got[:, :, 1] >= 2 ** n - 2).all()


def _raw_final_state_only(n, variant, solver, device, psi_bd, uniforms):
    """rydiff_forward with final_state_only through ctypes: one state out, shots at every save point."""
    amp, det, u, spec, tsave = _problem(n, variant, solver, device)
    batch = psi_bd.shape[0]
    psi = psi_bd.to(device).contiguous()
    call = _Call(spec, amp.to(torch.complex128).contiguous(), det, u, tsave.numpy(), batch, None)
    call.problem.final_state_only = 1
    u_dev = uniforms.to(device).contiguous()
    out = torch.full(tuple(u_dev.shape), -7, dtype=torch.int32, device=device)
    call.set_shots(np.arange(N_TSAVE, dtype=np.int32), u_dev, out)
    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=device)
    info = _native.RydPlanInfo()
    _native.check(L.rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()), stream, ctypes.byref(info)))
    ws = torch.empty(info.workspace_bytes, dtype=torch.uint8, device=device)
    last = torch.empty((1,) + tuple(psi.shape), dtype=torch.complex128, device=device)
    _native.check(L.rydiff_forward(ctypes.byref(call.problem), ctypes.byref(info), ctypes.c_void_p(psi.data_ptr()),
                                   ctypes.c_void_p(last.data_ptr()), None, ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(ws.numel()), 0, stream))
    torch.cuda.synchronize()
    return last, (out.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()


@pytest.mark.parametrize("n,variant,family,kernel,batch,solver", CASES, ids=IDS)
def test_no_stored_states_same_shots(cuda_device, evolved, n, variant, family, kernel, batch, solver):
    """store_states=False, final_state_only and need_tape = 1 with a gradient afterwards: bit-identical shots; the gradients are those
    of a run without shots.  (final_state_only is a launch-per-factor mode: the library refuses it on the one-launch sweeps up to
    12 qubits, shots or no shots, so it is exercised from 13 qubits on.)"""
    states, uniforms, want = evolved(n, variant, family, kernel, batch, solver)
    psi0 = _random_psi0(n, batch)
    request = ShotRequest(uniforms.shape[2], times="all", uniforms=uniforms)
    empty, got = _run(n, variant, solver, cuda_device, psi0, request, store_states=False, family=family, kernel=kernel)
    assert empty.numel() == 0 and (got == want).all()

    if n > 12:
        last, got = _raw_final_state_only(n, variant, solver, cuda_device, psi0, uniforms)
        assert (got == want).all() and float((last[0] - states[-1]).abs().max()) < 1e-13
    else:
        with pytest.raises(ValueError, match="final_state_only"):
            _raw_final_state_only(n, variant, solver, cuda_device, psi0, uniforms)

    zdiag = torch.arange(2 ** n, device=cuda_device).to(torch.float64)[None] / 2 ** n
    grads = []
    for with_shots in (True, False):
        amp, det, u, spec, tsave = _problem(n, variant, solver, cuda_device, store_states=False)
        spec.tape = "steps"  # one state per save point in the workspace tape: need_tape = 1
        request = ShotRequest(uniforms.shape[2], times="all", uniforms=uniforms)
        spec.shots = request if with_shots else None
        amp.requires_grad_(True)
        det.requires_grad_(True)
        _, expect = evolve(amp, det, u, tsave, psi0.to(cuda_device), spec, zdiag)
        assert spec.options["_last_stats"]["tape"] == "steps"
        if with_shots:
            torch.cuda.synchronize()
            assert (request.indices.cpu().numpy() == want).all()
        expect[0].sum().backward()
        torch.cuda.synchronize()
        grads.append((amp.grad.detach().cpu(), det.grad.detach().cpu()))
        assert float(grads[-1][0].abs().max()) > 0 and float(grads[-1][1].abs().max()) > 0
    for a, b in zip(*grads):
        assert float((a - b).abs().max()) <= ROUTE_TOL * float(b.abs().max())


def test_plan_reports_the_scratch(cuda_device):
    """rydiff_plan adds two doubles per 2^10 amplitudes and trajectory; up to 12 qubits also the trajectory the one-launch sweep is
    sampled from where the caller keeps none."""
    L = _native.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda_device).cuda_stream)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=cuda_device)
    for n, batch in ((9, 3), (14, 3)):
        amp, det, u, spec, tsave = _problem(n, 0, SolverType.KRYLOV_SE, cuda_device)
        sizes = []
        for with_shots in (False, True):
            call = _Call(spec, amp, det, u, tsave.numpy(), batch, None)
            if with_shots:
                call.set_shots(np.arange(N_TSAVE, dtype=np.int32), torch.zeros(N_TSAVE, batch, 8, dtype=torch.float64, device=cuda_device),
                               torch.zeros(N_TSAVE, batch, 8, dtype=torch.int32, device=cuda_device))
            info = _native.RydPlanInfo()
            _native.check(L.rydiff_plan(ctypes.byref(call.problem), 0, 0, ctypes.c_void_p(scratch.data_ptr()), stream, ctypes.byref(info)))
            sizes.append(info.workspace_bytes)
        chunks = max(2 ** n // 1024, 1)
        least = 2 * batch * chunks * 8 + (N_TSAVE * batch * 2 ** n * 16 if n <= 12 else 0)
        assert least <= sizes[1] - sizes[0] <= least + 3 * 256, (n, sizes)  # (every region is padded to 256 bytes)


# ---- the emulator ------------------------------------------------------------------------------------------------------------
def _pi_pulse_sequence(omega):
    """Three atoms a millimetre apart (interaction ~1e-11 rad/us: they do not see each other) under one resonant constant pulse."""
    reg = pl.Register.from_coordinates([[0.0, 0.0], [1000.0, 0.0], [2000.0, 0.0]])
    seq = pl.Sequence(reg, pl.MockDevice)
    seq.declare_channel("g", "rydberg_global")
    seq.add(pl.Pulse.ConstantPulse(200, omega, 0.0, 0.0), "g")
    return seq


TIMES = [0.05, 0.1, 0.15]


def _calibrated_pi_pulse():
    """The amplitude at which the emulator's own discretisation of the pulse is a pi rotation: resonant, phase-free and without
    interaction H(t) commutes with itself, so the rotation angle is proportional to the amplitude; it is read off a run at about
    pi / 2 (|<rrr|psi>| = sin^3, |<ggg|psi>| = cos^3 of half the angle) and scaled."""
    omega0 = 0.5 * np.pi / 0.2
    final = P.TorchEmulator.from_sequence(_pi_pulse_sequence(omega0), evaluation_times=TIMES).run(solver=SolverType.DP5_SE).states[-1, :, 0]
    theta0 = 2.0 * np.arctan2(float(final[0].abs()) ** (1 / 3), float(final[-1].abs()) ** (1 / 3))
    assert abs(theta0 - 0.5 * np.pi) < 0.05
    return omega0 * np.pi / theta0


def test_run_noisy_with_native_shots(cuda_device):
    """3 atoms, SPAM with eta = epsilon = epsilon_prime = 0 next to Doppler noise at zero temperature (what makes the emulator average
    over runs), a pi pulse: every count of the native route lands where the coherent run puts the weight — '000' at t = 0, '111'
    at the end — and every evaluation time holds runs x samples_per_run counts."""
    seq = _pi_pulse_sequence(_calibrated_pi_pulse())
    clean = P.TorchEmulator.from_sequence(seq, evaluation_times=TIMES).run(solver=SolverType.DP5_SE)
    assert isinstance(clean, CoherentResults)
    p_final = clean.states[-1, :, 0].abs() ** 2
    assert float(p_final[1:].sum()) < 1e-15  # a pi pulse to rounding: the other outcomes lie below the resolution of u * S
    cfg = P.SimConfig(noise=("SPAM", "doppler"), eta=0.0, epsilon=0.0, epsilon_prime=0.0, temperature=0.0, runs=5, samples_per_run=40)
    sim = P.TorchEmulator.from_sequence(seq, config=cfg, evaluation_times=TIMES)
    sim._noisy_state_budget = 2 * (8 + 5) * 8 * 16 + 2 * 5 * 40 * 12  # two runs per batch: three solver calls for the 5 runs
    torch.manual_seed(5)
    res = sim.run(solver=SolverType.DP5_SE, native_shots=True)
    assert isinstance(res, NoisyResults) and res.n_measures == 200 and len(res) == len(clean) == 5
    for k in range(len(res)):
        counts = res[k].bitstring_counts
        assert sum(counts.values()) == 5 * 40
        likely = {bits for bits, p in clean[k].sampling_dist.items() if p > 1e-12}
        assert set(counts) <= likely, (k, counts)
    assert dict(res[0].bitstring_counts) == {"000": 200} and dict(res[-1].bitstring_counts) == {"111": 200}
    # same seed, same shots: torch's generator governs the native route
    torch.manual_seed(5)
    again = sim.run(solver=SolverType.DP5_SE, native_shots=True)
    assert [dict(r.bitstring_counts) for r in again] == [dict(r.bitstring_counts) for r in res]
    # the default route still measures the same certain outcomes
    res = sim.run(solver=SolverType.DP5_SE)
    assert dict(res[0].bitstring_counts) == {"000": 200} and dict(res[-1].bitstring_counts) == {"111": 200}


def test_coherent_run_with_shots_and_no_stored_states(cuda_device):
    """run(shots=...) end to end: the shots of a store_states=False run are those the host reference draws from the stored states of
    the same sequence with the same uniforms (bracketed: the two runs' states agree to rounding), sample_final_state returns them,
    other counts and times fall back or say how to ask."""
    reg = pl.Register.rectangle(1, 4, spacing=8, prefix="q")
    seq = pl.Sequence(reg, pl.MockDevice)
    seq.declare_channel("g", "rydberg_global")
    seq.add(pl.Pulse(pl.BlackmanWaveform(300, 2.4), pl.RampWaveform(300, -3.0, 2.0), 0.0), "g")
    sim = P.TorchEmulator.from_sequence(seq, evaluation_times=[0.1, 0.2])
    stored = sim.run(solver=SolverType.KRYLOV_SE)
    torch.manual_seed(21)
    res = sim.run(solver=SolverType.KRYLOV_SE, store_states=False, shots=500)
    req = res.native_shots
    assert req.time_indices == (3,) and req.indices.shape == (1, 1, 500)
    torch.manual_seed(21)
    assert torch.equal(req.last_uniforms, torch.rand(1, 1, 500, dtype=torch.float64, device=cuda_device))
    _check_bracket(4, stored._states_tbd[-1:], req.last_uniforms.cpu(), req.indices.cpu().numpy())
    counts = res.sample_final_state(500)
    outcomes = indices_to_bitstrings(req.indices[0, 0].cpu(), "ground-rydberg", "ground-rydberg", 4)
    assert sum(counts.values()) == 500 and counts == {format(int(v), "04b"): int(c) for v, c in zip(*np.unique(outcomes.numpy(), return_counts=True))}
    assert set(counts) <= set(stored[-1].sampling_dist)
    with pytest.raises(RuntimeError, match=r"shots=ShotRequest\("):
        res.sample_final_state(100)
    with pytest.raises(RuntimeError, match=r"shots=ShotRequest\("):
        res.sample_state(0.1, 500)
    every = sim.run(solver=SolverType.KRYLOV_SE, store_states=False, shots=ShotRequest(50, times="all"))
    assert every.sample_state(0.0, 50) == {"0000": 50} and sum(every.sample_state(0.1, 50).values()) == 50
    with pytest.raises(NotImplementedError, match="master-equation"):
        sim.run(solver=SolverType.DP5_ME, shots=10)
    # shots next to a gradient: a non-differentiable by-product
    sim2 = P.TorchEmulator.from_sequence(seq, evaluation_times=[0.1, 0.2])
    z = P.DiagonalObservable(torch.arange(16, dtype=torch.float64))
    out = sim2.run(solver=SolverType.KRYLOV_SE, time_grad=True, observables=[z], store_states=False, shots=20)
    out.expect([z])[0].real[-1].backward()
    assert sim2.evaluation_times.grad is not None and sum(out.sample_final_state(20).values()) == 20


def test_three_level_basis(cuda_device):
    """Basis "all", 2 atoms (two qubits per atom natively): the native shots stay on the populated codes and their bitstrings are
    outcomes the stored-state result can produce."""
    from tests.test_host_logic import _three_level_emulator

    sim, _ = _three_level_emulator(compute_device="cuda", n=2)
    stored = sim.run(solver=SolverType.KRYLOV_SE)
    torch.manual_seed(8)
    res = sim.run(solver=SolverType.KRYLOV_SE, store_states=False, shots=400)
    idx = res.native_shots.indices[0, 0].cpu()
    valid = set(sim._hamiltonian.embedded_three_level().tolist())
    assert set(idx.tolist()) <= valid and len(set(idx.tolist())) > 1
    counts = res.sample_final_state(400)
    assert sum(counts.values()) == 400 and set(counts) <= set(stored[-1].sampling_dist)
    # bracket against the stored 3^n state scattered into the 4^n register
    big = torch.zeros(1, 1, 16, dtype=torch.complex128)
    big[0, 0, sim._hamiltonian.embedded_three_level()] = stored._states_tbd[-1, 0].cpu()
    _check_bracket(4, big, res.native_shots.last_uniforms.cpu(), res.native_shots.indices.cpu().numpy())
