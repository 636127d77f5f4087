"""Cost of native measurement shots against the route through stored states (profiles/native_shots.txt):
    python tools/time_shots.py [N] [T] [shots] [mode] [timeout_s]

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments), T steps
(T + 1 evaluation times), KRYLOV_SE, one trajectory; `shots` measurement shots at EVERY evaluation time.  Legs:
  a  forward, nothing stored, no shots (the floor both routes stand on)
  n  native: store_states=False with a ShotRequest at all times
  s  stored states (what the parent commit offers): store_states=True, |psi|^2 on the device, torch.multinomial per call
mode "time":    one warm-up per leg, then ROUNDS timed calls per leg, alternated; each call is closed by a synchronise; medians.
                The peak torch.cuda.max_memory_allocated of one call of n and of s follows.
mode "profile": three calls of n with ONE overlap target next to the shots and nothing else — the workload of a
                `rocprofv3 --kernel-trace --stats` run of its own: k_shot_chunk_sums (pass A: one read of the state) and
                k_overlap_expect<1> (one read of the state and one of the target) then run on the same states.
The script ends itself after `timeout_s` seconds (default 300)."""
import gc
import signal
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

gc.collect()
gc.freeze()
from pulser_diff_amd.shots import ShotRequest  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
n_shots = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
mode = sys.argv[4] if len(sys.argv) > 4 else "time"
signal.alarm(int(sys.argv[5]) if len(sys.argv) > 5 else 300)  # SIGALRM ends the process
ROUNDS = 7
dev = torch.device("cuda")
rows = 4 if n % 4 == 0 else 1
coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows) for j in range(n // rows)], dtype=torch.float64)
iu = torch.triu_indices(n, n, 1)
u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev)
params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev)
seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
amp = (0.5 * params[:4][seg])[None, None, :].contiguous()  # real: a drive without phase
det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
psi0[:, -1] = 1
ts = torch.arange(T + 1, dtype=torch.float64) / 1000
mask = (1 << n) - 1


def spec_of(store, shots=None, overlaps=None):
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=store, shots=shots, overlaps=overlaps)


def leg_a():
    with torch.no_grad():
        evolve(amp, det, u, ts, psi0, spec_of(False), None)


def leg_n(overlaps=None):
    req = ShotRequest(n_shots, times="all")
    with torch.no_grad():
        evolve(amp, det, u, ts, psi0, spec_of(False, req, overlaps), None)
    return req.indices[:, 0]  # (T + 1, shots)


def leg_s():
    with torch.no_grad():
        states, _ = evolve(amp, det, u, ts, psi0, spec_of(True), None)
        probs = states.real**2 + states.imag**2
        del states
        return torch.multinomial(probs[:, 0, :], n_shots, replacement=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


if mode == "profile":
    target = torch.randn(2**n, generator=torch.Generator().manual_seed(0), dtype=torch.complex128)
    packed = (target / target.norm()).to(dev)[None, None, :].contiguous()
    for _ in range(3):
        leg_n(packed)
    torch.cuda.synchronize()
    sys.exit(0)

LEGS = {"a": leg_a, "n": leg_n, "s": leg_s}
for fn in LEGS.values():  # one warm-up each
    fn()
torch.cuda.synchronize()
times = {k: [] for k in LEGS}
for _ in range(ROUNDS):
    for name, fn in LEGS.items():
        times[name].append(timed(fn))
        if name == "s":
            torch.cuda.empty_cache()
med = {k: statistics.median(v) for k, v in times.items()}
print(f"N={n} T={T} ({T + 1} evaluation times) shots={n_shots} per time, B=1  ({ROUNDS} timed calls per leg after one warm-up; median ms, min .. max)")
for k, label in (("a", "forward, nothing stored, no shots"), ("n", "native shots, store_states=False"), ("s", "stored states + |psi|^2 + torch.multinomial")):
    print(f"  leg {k}: {med[k] * 1e3:9.3f} ms   ({min(times[k]) * 1e3:.3f} .. {max(times[k]) * 1e3:.3f})   {label}")
print(f"  per evaluation time above leg a: native {(med['n'] - med['a']) / (T + 1) * 1e6:.2f} us   stored {(med['s'] - med['a']) / (T + 1) * 1e6:.2f} us")
for name, fn in (("n (native)", leg_n), ("s (stored states)", leg_s)):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"  leg {name}: peak allocated {peak / 2**20:.1f} MiB ({(peak - base) / 2**20:.1f} MiB above the {base / 2**20:.1f} MiB held before)")
