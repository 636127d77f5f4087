"""All-times sensitivities of NOISY runs: the tangent sweep on the doubled register against the loop of one-hot reverse sweeps, both
through TorchEmulator.run_sensitivities(route=...) in the same process (profiles/dm_tangent_sweep.txt):
    python tools/time_dm_tangent.py N_ATOMS N_T D N_OBS        (N_T: 21 | 101 ...; D: 2 | 8; N_OBS: 1 | 4)

Shape: N_ATOMS atoms on a line 8 um apart, a Blackman pulse (400 ns) with a detuning ramp followed by a constant pulse (400 ns), global
channel, dephasing + relaxation (the dissipator block has the diagonal and the double flip), sampling rate 0.25, N_T evaluation
times.  D = 2: the constant pulse's amplitude and the Blackman area; D = 8: those, both ends of the detuning ramp and the coordinates
of two atoms.  N_OBS = 1: sum Z; 4: sum Z, sum X (Pauli), a fidelity <phi|rho|phi> and the purity.  Legs:
  tangent  run_sensitivities(route="tangent"): ceil(D / 8) sweeps of 1 + D vectors of 4^N amplitudes
  loop     run_sensitivities(route="adjoint-loop"): one differentiated master-equation run, then N_OBS * N_T reverse sweeps
tangent: median of 3 windows of at least 0.2 s after a warm run; loop: the call that is compared with the sweep, then ONE timed call
(where the first took 20 s or more it is the figure reported: warm-up is then below a percent of it).
The two routes are compared before anything is timed (1e-8 relative to the largest entry of each observable's derivatives).

Traffic model of one factor pass of the sweep: (1 + D) vectors read and written once, (1 + D) * (R + W) * 16 * 4^N bytes with
R + W = 2; partner reads (flip bits, pair terms) are cache traffic and are NOT counted.  The pass count is total_factors of the plan
(results.solver_stats of a plain run of the same emulator); the achieved GB/s divides the model's bytes by the WHOLE tangent call
(host-side table tangents, observable launches and planning included), so it is a lower bound of the kernel's own rate.

One process per shape, every one under its own time limit, chained so that trouble ends the chain:
    timeout -k 10 120 python tools/time_dm_tangent.py 3 21 2 1 && timeout -k 10 120 python tools/time_dm_tangent.py 3 21 8 4 && ..."""
import gc
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

gc.collect()
gc.freeze()
import pulser_diff_amd as P  # noqa: E402
from pulser_diff_amd import pulses as pl  # noqa: E402
from pulser_diff_amd.observables import PauliObservable, Purity, StateOverlap  # noqa: E402
from pulser_diff_amd.utils import DiagonalObservable, total_magnetization_diag  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_t = int(sys.argv[2]) if len(sys.argv) > 2 else 21
D = int(sys.argv[3]) if len(sys.argv) > 3 else 2
n_obs = int(sys.argv[4]) if len(sys.argv) > 4 else 1
assert D in (2, 8) and n_obs in (1, 4) and n >= 2
dev = torch.device("cuda")
f64 = lambda v, grad=True: torch.tensor(v, dtype=torch.float64, requires_grad=grad)  # noqa: E731

coords = {f"q{j}": f64([8.0 * j, 0.0], grad=(D == 8 and j < 2)) for j in range(n)}
omega, area, det0, det1 = f64([5.0]), f64([torch.pi]), f64([-5.0], D == 8), f64([2.0], D == 8)
seq = pl.Sequence(pl.Register(coords), pl.MockDevice)
seq.declare_channel("rydberg_global", "rydberg_global")
seq.add(pl.Pulse(pl.BlackmanWaveform(400, area), pl.RampWaveform(400, det0, det1), 0.3), "rydberg_global")
seq.add(pl.Pulse.ConstantPulse(400, omega, 0.0, 0.3), "rydberg_global")
cfg = P.SimConfig(noise=("dephasing", "relaxation"), dephasing_rate=0.5, relaxation_rate=0.3)
times = [0.8 * k / (n_t - 1) for k in range(1, n_t - 1)]  # (t = 0 and the end are added by the emulator)
sim = P.TorchEmulator.from_sequence(seq, sampling_rate=0.25, config=cfg, evaluation_times=times, compute_device=dev)
assert len(sim.evaluation_times) == n_t, len(sim.evaluation_times)
x = [omega, area] + ([det0, det1, coords["q0"], coords["q1"]] if D == 8 else [])
assert sum(t.numel() for t in x) == D

gen = torch.Generator().manual_seed(7)
target = torch.randn(2**n, generator=gen, dtype=torch.complex128)
obs = [DiagonalObservable(total_magnetization_diag(n))]
if n_obs == 4:
    obs += [PauliObservable(n, [(1.0, {j: "X"}) for j in range(n)]), StateOverlap(target / target.norm()), Purity()]


def leg(route):
    return sim.run_sensitivities(x, obs, route=route)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


# the two routes give the same numbers (this also warms every shape)
tan = leg("tangent")
torch.cuda.synchronize()
t0 = time.perf_counter()
loop = leg("adjoint-loop")
torch.cuda.synchronize()
t_loop_first = time.perf_counter() - t0
assert tan.route == "tangent" and loop.route == "adjoint-loop"
err = 0.0
for o in range(n_obs):
    scale = max(float(g[o].abs().max()) for g in loop.grads)
    err = max(err, max(float((a[o].cpu() - b[o].cpu()).abs().max()) for a, b in zip(tan.grads, loop.grads)) / scale)
assert err < 1e-8, f"tangent sweep and adjoint loop disagree: {err:.2e}"
del tan, loop
passes = int(sim.run(store_states=False, observables=obs[:1]).solver_stats["total_factors"])

reps = max(1, int(0.2 / max(window(lambda: leg("tangent"), 1), 1e-6)) + 1)
t_tan = statistics.median(window(lambda: leg("tangent"), reps) for _ in range(3))
t_loop = window(lambda: leg("adjoint-loop"), 1) if t_loop_first < 20.0 else t_loop_first  # (a long loop is not run twice)
model_bytes = passes * (1 + D) * 2 * 16 * 4**n
print(f"atoms={n:2d} n_t={n_t:3d} D={D} n_obs={n_obs}:  tangent {t_tan * 1e3:10.3f} ms   adjoint loop {t_loop * 1e3:11.3f} ms   "
      f"loop / tangent {t_loop / t_tan:7.2f}   factor passes {passes:5d}   {model_bytes / 1e6:10.2f} MB per sweep, "
      f"{model_bytes / t_tan / 1e9:8.2f} GB/s over the whole call   (routes agree to {err:.1e})")
