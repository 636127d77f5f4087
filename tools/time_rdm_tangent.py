"""Cost of the reduced-density-matrix tangents of the tangent sweep (profiles/rdm_tangent.txt):
    python tools/time_rdm_tangent.py [N] [T] [m]

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments), T steps,
KRYLOV_SE, D = 4 directions (one per segment of the amplitude table), one subsystem of m qubits spread over the register (qubit 0 and
qubit N - 1 among them from m = 3 on; default: m = 1 and m = 6, one after the other).  Legs, alternated inside every round and timed
with device events around whole runs:
  (b) sweep     the tangent sweep, one diagonal row (so that dexpect_out exists), no RDM
  (a) sweep+rdm the same sweep with the RDM rows: per save point (a - b) / (T + 1) = one k_rdm_expect launch and one k_rdm_tangent
                launch over the 4 directions; the achieved bytes/s are 2 D 2^N 16 B (the derived traffic of k_rdm_tangent) plus
                2^N 16 B (k_rdm_expect) over that time
  (c) loop      what the reverse sweep offers for d purity(rho_A)(t_k) / d theta at all k: T + 1 times evolve + backward with the
                cotangent of purity at one save point (timed for 3 save points and scaled; every reverse sweep costs the same)
Every shape is warmed; a window holds enough repeats to last well above 0.2 s; the median of 5 rounds is reported."""
import gc
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

gc.collect()
gc.freeze()
from pulser_diff_amd import _native  # noqa: E402
from pulser_diff_amd.observables import ReducedDensityMatrix  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, evolve_tangent, split_observables  # noqa: E402
from pulser_diff_amd.utils import purity, purity_tangent  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
MS = [int(sys.argv[3])] if len(sys.argv) > 3 else [1, 6]
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
SUBS = {1: (n // 2,), 3: (0, n // 2, n - 1), 6: (0, n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5, n - 1)}


def spec_of(rdm=None):
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=False, rdms=None if rdm is None else [rdm])


def sweep(rdm=None):
    return evolve_tangent(amp, det, u, ts, psi0, spec_of(rdm), ones, d_amp=d_amp, flags=_native.TANGENT_RDMS if rdm is not None else 0)


def reverse_sweep(rdm, k):
    a = amp.clone().requires_grad_(True)
    expect = evolve(a, det, u, ts, psi0, spec_of(rdm), None)[1]
    rho = split_observables(expect, 0, [rdm])[2][0]
    purity(rho[k, 0]).backward()
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


for m in MS:
    rdm = ReducedDensityMatrix(SUBS[m])
    # the legs agree before they are timed: d purity / d params[j] at the last save point
    expect, dexpect = sweep(rdm)
    rho = split_observables(expect[1:], 0, [rdm])[2][0]
    tangent = torch.stack([purity_tangent(rho[-1, 0], split_observables(dexpect[j, 1:], 0, [rdm])[2][0][-1, 0]) for j in range(D)])
    adjoint = torch.stack([(reverse_sweep(rdm, T)[0, 0] * d_amp[j, 0, 0].conj()).real.sum() for j in range(D)])
    assert float((tangent - adjoint).abs().max()) <= 1e-8 * max(float(adjoint.abs().max()), 1e-6), "tangent sweep and reverse sweep disagree"
    points = [0, T // 2, T][:LOOP_POINTS]
    legs = {"sweep": lambda: sweep(), "sweep+rdm": lambda: sweep(rdm), "loop": lambda: [reverse_sweep(rdm, k) for k in points]}
    reps = {}
    for name, fn in legs.items():  # warm every shape, then size the windows
        fn()
        reps[name] = max(1, int(0.3 / max(window(fn, 1), 1e-6)) + 1)
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            times[name].append(window(fn, reps[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    print(f"N={n} T={T} B=1 D={D} m={m}  ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
    for k in legs:
        print(f"  leg {k:10s}: {med[k] * 1e3:10.3f} ms   spread {spread[k] * 100:5.1f} %   ({reps[k]} runs per window)")
    per = (med["sweep+rdm"] - med["sweep"]) / (T + 1)
    traffic = (2 * D + 1) * 2**n * 16
    loop = med["loop"] / len(points) * (T + 1)
    print(f"  (a) - (b) per save point: {per * 1e6:.2f} us for {traffic / 2**20:.2f} MiB of derived traffic = {traffic / max(per, 1e-12) * 1e-9:.1f} GB/s; "
          f"{16.0 * 2 ** (n + m) * D / max(per, 1e-12) * 1e-12:.2f} TFLOP/s of the 16 * 2^(N+m) * D estimate")
    print(f"  (a) all {T + 1} times, {D} directions: {med['sweep+rdm'] * 1e3:.3f} ms ({(med['sweep+rdm'] / med['sweep'] - 1) * 100:.1f} % over (b))   "
          f"(c) {T + 1} reverse sweeps: {loop * 1e3:.3f} ms   (c) / (a) = {loop / med['sweep+rdm']:.1f}")
