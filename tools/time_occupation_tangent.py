"""Cost of the occupation-correlation tangents of the tangent sweep (profiles/occupation_tangent.txt):
    python tools/time_occupation_tangent.py [N] [T]

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments), T steps,
KRYLOV_SE, D = 4 directions (one per segment of the amplitude table).  Legs, alternated inside every round and timed with device
events around whole runs:
  (b) sweep          the tangent sweep, one diagonal row (so that dexpect_out exists), no moments
  (a) sweep+moments  the same sweep with the Moments block: per save point (a - b) / (T + 1) = one k_moments_tile launch (values) and
                     one k_moments_tangent launch over the 4 directions (past 12 qubits each followed by k_moments_finish); the
                     achieved bytes/s are 2 D 2^N 16 B (the derived traffic of k_moments_tangent: psi is read again per direction)
                     plus 2^N 16 B (k_moments_tile) over that time
  (d) sweep+tables   the same sweep with the same 1 + N + N(N-1)/2 rows handed as diagonal tables (k_expect_tangent), where the
                     tables fit in 4 GiB
  (c) loop           what the reverse sweep offers for d structure_factor(t_k) / d theta at all k: T + 1 times evolve + backward with
                     the cotangent of the Neel structure factor at one save point (timed for 3 save points and scaled; every reverse
                     sweep costs the same)
and, on the public route (a chain of N atoms, a Blackman pulse and a constant one, x = [omega, delta, area]):
  (p) TorchEmulator.run_occupation_sensitivities(x).d_structure_factor(neel) at all n_t evaluation times
  (q) run(observables=[OccupationCorrelations()]) once and one autograd.grad of structure_factor(neel)[k] per k (3 timed, scaled)
Every shape is warmed; a window holds enough repeats to last well above 0.2 s; the median of 5 rounds is reported."""
import gc
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

gc.collect()
gc.freeze()
import pulser_diff_amd as P  # noqa: E402
import pulser_diff_amd.pulses as pl  # noqa: E402
from pulser_diff_amd import _native  # noqa: E402
from pulser_diff_amd.observables import OccupationCorrelations, moment_rows  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, evolve_tangent, split_moments  # noqa: E402
from pulser_diff_amd.utils import connected_correlations, structure_factor, structure_factor_tangent  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
D, ROUNDS, LOOP_POINTS = 4, 5, 3
dev = torch.device("cuda")
rows = 4 if n % 4 == 0 else 1
coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows) for j in range(n // rows)], dtype=torch.float64)
iu = torch.triu_indices(n, n, 1)
u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev)
params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev)
seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
psi0[:, -1] = 1
ts = torch.arange(T + 1, dtype=torch.float64) / 1000
mask = (1 << n) - 1
amp = (0.5 * params[:4][seg])[None, None, :].to(torch.complex128).contiguous()
det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
d_amp = torch.stack([0.5 * (seg == j).to(torch.complex128) for j in range(D)])[:, None, None, :].contiguous()  # d amp / d params[j]
ones = torch.ones(1, 2**n, dtype=torch.float64, device=dev)
neel = [(-1.0) ** i for i in range(n)]
n_rows = moment_rows(n)
tables = None
if n_rows * 2**n * 8 <= 4 * 2**30:  # the rows as diagonal tables: S, y_q, y_q y_r in the order of the Moments block
    y = torch.arange(2**n, device=dev)
    bit = [((y >> (n - 1 - q)) & 1).to(torch.float64) for q in range(n)]
    tables = torch.stack([ones[0]] + bit + [bit[q] * bit[r] for q in range(n) for r in range(q + 1, n)])
    del bit


def spec_of(moments):
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=False, moments=moments)


def sweep(moments=False, diag=ones):
    return evolve_tangent(amp, det, u, ts, psi0, spec_of(moments), diag, d_amp=d_amp, flags=_native.TANGENT_MOMENTS if moments else 0)


def reverse_sweep(k):
    a = amp.clone().requires_grad_(True)
    mom = evolve(a, det, u, ts, psi0, spec_of(True), None)[1]
    structure_factor(connected_correlations(mom[:, k, 0], n), neel).backward()
    return a.grad


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / reps


def timed(legs):
    reps = {}
    for name, fn in legs.items():  # warm every shape, then size the windows
        fn()
        reps[name] = max(1, int(0.3 / max(window(fn, 1), 1e-6)) + 1)
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            times[name].append(window(fn, reps[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"  leg {k:14s}: {med[k] * 1e3:10.3f} ms   spread {(max(v) - min(v)) / med[k] * 100:5.1f} %   ({reps[k]} runs per window)")
    return med


# the legs agree before they are timed: d structure factor / d params[j] at the last save point, and the table rows
expect, dexpect = sweep(True)
mom, dmom = split_moments(expect, n)[1], torch.stack([split_moments(dexpect[j], n)[1] for j in range(D)], dim=1)
tangent = structure_factor_tangent(mom[:, -1, 0], dmom[:, :, -1, 0], n, neel)
adjoint = torch.stack([(reverse_sweep(T)[0, 0] * d_amp[j, 0, 0].conj()).real.sum() for j in range(D)])
assert float((tangent - adjoint).abs().max()) <= 1e-8 * max(float(adjoint.abs().max()), 1e-6), "tangent sweep and reverse sweep disagree"
if tables is not None:
    drows = sweep(False, tables)[1]
    assert float((drows - dexpect[:, 1:]).abs().max()) <= 1e-10 * float(drows.abs().max()), "native rows and diagonal-table rows disagree"
    del drows
points = [0, T // 2, T][:LOOP_POINTS]
legs = {"sweep": lambda: sweep(), "sweep+moments": lambda: sweep(True)}
if tables is not None:
    legs["sweep+tables"] = lambda: sweep(False, tables)
legs["loop"] = lambda: [reverse_sweep(k) for k in points]
print(f"N={n} T={T} B=1 D={D} rows={n_rows}  ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
med = timed(legs)
per = (med["sweep+moments"] - med["sweep"]) / (T + 1)
traffic = (2 * D + 1) * 2**n * 16
loop = med["loop"] / len(points) * (T + 1)
print(f"  (a) - (b) per save point: {per * 1e6:.2f} us for {traffic / 2**20:.2f} MiB of derived traffic ((2 D + 1) state reads) = "
      f"{traffic / max(per, 1e-12) * 1e-9:.1f} GB/s")
print(f"  (a) all {T + 1} times, {D} directions: {med['sweep+moments'] * 1e3:.3f} ms ({(med['sweep+moments'] / med['sweep'] - 1) * 100:.1f} % over (b))   "
      f"(c) {T + 1} reverse sweeps: {loop * 1e3:.3f} ms   (c) / (a) = {loop / med['sweep+moments']:.1f}")
if tables is not None:
    print(f"  (d) the same rows as {n_rows} diagonal tables: {med['sweep+tables'] * 1e3:.3f} ms   ((d) - (b)) / ((a) - (b)) = "
          f"{(med['sweep+tables'] - med['sweep']) / max(med['sweep+moments'] - med['sweep'], 1e-12):.1f}")
del tables

# ---- the public route -------------------------------------------------------------------------------------------------------------
f64 = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)  # noqa: E731
area, omega, delta = f64([3.0]), f64([4.0]), f64([1.0])
seq = pl.Sequence(pl.Register.rectangle(1, n, torch.tensor([7.0], dtype=torch.float64)), pl.MockDevice)
seq.declare_channel("ch", "rydberg_global")
seq.add(pl.Pulse(pl.BlackmanWaveform(400, area), pl.RampWaveform(400, -2.0, delta), 0), "ch")
seq.add(pl.Pulse.ConstantPulse(200, omega, delta, 0.0), "ch")
sim = P.TorchEmulator.from_sequence(seq, sampling_rate=0.1, evaluation_times=0.25, compute_device=dev)
x = [omega, delta, area]
n_t = len(sim.evaluation_times)
pub_points = [0, n_t // 2, n_t - 1]


def public_sweep():
    return sim.run_occupation_sensitivities(x, solver=SolverType.KRYLOV_SE).d_structure_factor(neel)


def public_loop():
    f = sim.run(solver=SolverType.KRYLOV_SE, observables=[OccupationCorrelations()], store_states=False).structure_factor(neel)
    return [torch.autograd.grad(f[k], x, retain_graph=True) for k in pub_points]


got, want = public_sweep(), public_loop()
for i in range(3):
    ref = torch.stack([want[j][i][0] for j in range(len(pub_points))]).cpu()
    assert float((got[i][pub_points, 0, 0].cpu() - ref).abs().max()) <= 1e-8 * max(float(ref.abs().max()), 1e-6), "public routes disagree"
print(f"public route: chain of {n} atoms, {n_t} evaluation times, 3 parameters")
med = timed({"sensitivities": public_sweep, "run+3 grads": public_loop, "run": lambda: sim.run(
    solver=SolverType.KRYLOV_SE, observables=[OccupationCorrelations()], store_states=False).structure_factor(neel)})
grad = (med["run+3 grads"] - med["run"]) / len(pub_points)
loop = med["run"] + grad * n_t
print(f"  (p) d structure factor at all {n_t} times: {med['sensitivities'] * 1e3:.3f} ms   (q) run + {n_t} reverse sweeps: {loop * 1e3:.3f} ms   "
      f"(q) / (p) = {loop / med['sensitivities']:.1f}")
