"""Cost of the native Pauli-string observables (profiles/pauli_observables.txt): python tools/time_pauli_observables.py [N] [T] [B]

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments, 8 pulse
parameters), T steps, KRYLOV_SE, observable <sum_j X_j> (N strings, N flip masks).  Legs, alternated inside every round:
  a  forward, no observable                    b  a + the diagonal sum Z table (fused reduction; context)
  c  a + native <sum X>, automatic choice      d  a + native <sum X>, direct evaluation only (kernel variant 1 evaluates the
                                                  observable AND runs the factor passes on the direct kernels: d0 is its own baseline)
  e  store_states=True, then the same sum formed by torch index arithmetic from the stored states (what the parent commit offers)
  f  forward + gradient of <sum X>(T) w.r.t. the 8 pulse parameters, native      g  the same through stored states and grad_states
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
from pulser_diff_amd.observables import PauliObservable, expect_pauli  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
B = int(sys.argv[3]) if len(sys.argv) > 3 else 1
ROUNDS = 5
dev = torch.device("cuda")
rows = 4 if n % 4 == 0 else 1
coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows) for j in range(n // rows)], dtype=torch.float64)
iu = torch.triu_indices(n, n, 1)
u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev)
params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev, requires_grad=True)
seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
psi0 = torch.zeros(B, 2**n, dtype=torch.complex128, device=dev)
psi0[:, -1] = 1
ts = torch.arange(T + 1, dtype=torch.float64) / 1000
mask = (1 << n) - 1
sum_x = PauliObservable(n, [(1.0, {j: "X"}) for j in range(n)])
x = torch.arange(2**n, device=dev)
zdiag = sum((1.0 - 2.0 * ((x >> j) & 1).to(torch.float64)) for j in range(n))[None]


def tables():
    amp = (0.5 * params[:4][seg])[None, None, :].expand(B, 1, T + 1).contiguous()  # real: a drive without phase
    det = (-0.5 * params[4:][seg])[None, None, :].expand(B, 1, T + 1).contiguous()
    return amp, det


def spec_of(store, pauli=None, variant=0):
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=store, pauli=pauli,
                       kernel_variant=variant)


def forward(store=False, pauli=None, obs=None, variant=0):
    with torch.no_grad():
        amp, det = tables()
        return evolve(amp, det, u, ts, psi0, spec_of(store, pauli, variant), obs)


def leg_e():
    states, _ = forward(store=True)
    return torch.stack([expect_pauli(sum_x, states[:, b, :, None]).real for b in range(B)])


def leg_f():
    amp, det = tables()
    _, e = evolve(amp, det, u, ts, psi0, spec_of(False, [sum_x]), None)
    return torch.autograd.grad(e[0, -1].sum(), params)[0]


def leg_g():
    amp, det = tables()
    states, _ = evolve(amp, det, u, ts, psi0, spec_of(True), None)
    last = sum(expect_pauli(sum_x, states[-1:, b, :, None]).real for b in range(B))
    return torch.autograd.grad(last.sum(), params)[0]


LEGS = {"a": lambda: forward(), "b": lambda: forward(obs=zdiag), "c": lambda: forward(pauli=[sum_x]),
        "d0": lambda: forward(variant=1), "d": lambda: forward(pauli=[sum_x], variant=1), "e": leg_e, "f": leg_f, "g": leg_g}


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


reps = {}
for name, fn in LEGS.items():  # warm every shape, then size the windows
    fn()
    one = window(fn, 1)
    reps[name] = max(1, int(0.3 / max(one, 1e-6)) + 1)
ce = forward(pauli=[sum_x])[1][0, :, 0]
assert (ce - leg_e()[0]).abs().max().item() < 1e-9, "native and stored-state values disagree"
assert (leg_f() - leg_g()).abs().max().item() < 1e-8 * max(1.0, leg_g().abs().max().item()), "native and stored-state gradients disagree"
times = {k: [] for k in LEGS}
for _ in range(ROUNDS):
    for name, fn in LEGS.items():
        times[name].append(window(fn, reps[name]))
        if name in ("e", "g"):
            torch.cuda.empty_cache()
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
print(f"N={n} T={T} B={B}  ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
for k in LEGS:
    print(f"  leg {k:2s}: {med[k] * 1e3:9.3f} ms   spread {spread[k] * 100:5.1f} %   ({reps[k]} runs per window)")
per = lambda a, b: (med[a] - med[b]) / (T + 1) * 1e6  # noqa: E731
print(f"  per save point: c - a = {per('c', 'a'):.2f} us   d - d0 = {per('d', 'd0'):.2f} us   e - a = {per('e', 'a'):.2f} us   b - a = {per('b', 'a'):.2f} us")
print(f"  gradient of <sum X>(T): f = {med['f'] * 1e3:.3f} ms   g = {med['g'] * 1e3:.3f} ms")
print(f"  acceptance: c < e: {med['c'] < med['e']}   f < g: {med['f'] < med['g']}   c - a <= d - d0: {per('c', 'a') <= per('d', 'd0')}")
