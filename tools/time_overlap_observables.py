"""Cost of the native state-overlap observables (profiles/overlap_observables.txt):
    python tools/time_overlap_observables.py [N] [T] [mode]

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments, 8 pulse
parameters), T steps, KRYLOV_SE, one target (a random normalised vector).  Legs, alternated inside every round:
  a  forward, no observable                    c  a + the native overlap at every save point
  e  store_states=True, then torch's target.conj() @ states (what the parent commit offers)
  f  forward + gradient of 1 - |c(T)|^2 w.r.t. the 8 pulse parameters, native      g  the same through stored states and grad_states
mode "profile": four runs of f with the loss 1 - mean_k |c(t_k)|^2 and nothing else (the workload of a rocprofv3 --kernel-trace
                --stats run of its own);
mode "memory":  peak torch.cuda.max_memory_allocated of one f and of one g.
Every shape is warmed; a window is closed by a synchronise and holds enough repeats to last well above 0.2 s."""
import gc
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

gc.collect()
gc.freeze()
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, split_expect  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
mode = sys.argv[3] if len(sys.argv) > 3 else "time"
ROUNDS = 5
dev = torch.device("cuda")
rows = 4 if n % 4 == 0 else 1
coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows) for j in range(n // rows)], dtype=torch.float64)
iu = torch.triu_indices(n, n, 1)
u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev)
params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev, requires_grad=True)
seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
psi0[:, -1] = 1
ts = torch.arange(T + 1, dtype=torch.float64) / 1000
mask = (1 << n) - 1
target = torch.randn(2**n, generator=torch.Generator().manual_seed(0), dtype=torch.complex128)
target = (target / target.norm()).to(dev)
packed = target[None, None, :].contiguous()  # (n_ov, 1, dim)


def tables():
    amp = (0.5 * params[:4][seg])[None, None, :].contiguous()  # real: a drive without phase
    det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
    return amp, det


def spec_of(store, overlaps=None):
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=store, overlaps=overlaps)


def forward(store=False, overlaps=None):
    with torch.no_grad():
        amp, det = tables()
        return evolve(amp, det, u, ts, psi0, spec_of(store, overlaps), None)


def leg_c():
    return split_expect(forward(overlaps=packed)[1], 1)[1][0, :, 0]


def leg_e():
    states, _ = forward(store=True)
    return states[:, 0, :] @ target.conj()


def leg_f(every_save_point=False):
    amp, det = tables()
    _, e = evolve(amp, det, u, ts, psi0, spec_of(False, packed), None)
    c = split_expect(e, 1)[1]
    loss = (c[0, :, 0].abs() ** 2).mean() if every_save_point else c[0, -1, 0].abs() ** 2
    return torch.autograd.grad(1 - loss, params)[0]


def leg_g():
    amp, det = tables()
    states, _ = evolve(amp, det, u, ts, psi0, spec_of(True), None)
    return torch.autograd.grad(1 - torch.vdot(target, states[-1, 0]).abs() ** 2, params)[0]


LEGS = {"a": lambda: forward(), "c": leg_c, "e": leg_e, "f": leg_f, "g": leg_g}


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


if mode == "profile":
    for _ in range(4):
        leg_f(every_save_point=True)  # a cotangent at every save point: no call of k_overlap_apply takes its zero shortcut
    torch.cuda.synchronize()
    sys.exit(0)
if mode == "memory":
    for name, fn in (("f (native)", leg_f), ("g (stored states)", leg_g)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(f"N={n} T={T} leg {name}: peak allocated {peak / 2**20:.1f} MiB ({(peak - base) / 2**20:.1f} MiB above the {base / 2**20:.1f} MiB held before)")
    sys.exit(0)

reps = {}
for name, fn in LEGS.items():  # warm every shape, then size the windows
    fn()
    one = window(fn, 1)
    reps[name] = max(1, int(0.3 / max(one, 1e-6)) + 1)
assert (leg_c() - leg_e()).abs().max().item() < 1e-9, "native and stored-state values disagree"
assert (leg_f() - leg_g()).abs().max().item() < 1e-8 * max(1.0, leg_g().abs().max().item()), "native and stored-state gradients disagree"
times = {k: [] for k in LEGS}
for _ in range(ROUNDS):
    for name, fn in LEGS.items():
        times[name].append(window(fn, reps[name]))
        if name in ("e", "g"):
            torch.cuda.empty_cache()
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
print(f"N={n} T={T} B=1  ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
for k in LEGS:
    print(f"  leg {k:2s}: {med[k] * 1e3:9.3f} ms   spread {spread[k] * 100:5.1f} %   ({reps[k]} runs per window)")
per = lambda a, b: (med[a] - med[b]) / (T + 1) * 1e6  # noqa: E731
print(f"  per save point: c - a = {per('c', 'a'):.2f} us   e - a = {per('e', 'a'):.2f} us")
print(f"  gradient of 1 - |c(T)|^2: f = {med['f'] * 1e3:.3f} ms   g = {med['g'] * 1e3:.3f} ms")
