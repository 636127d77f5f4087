"""Cost of the native occupation correlations (profiles/occupation_moments.txt):
    python tools/time_occupation_moments.py [N] [T] [mode]

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments), T steps,
KRYLOV_SE, B = 1, psi0 = all ground.  All legs serve the same 1 + N + N(N-1)/2 rows; alternated inside every round:
  a  forward, no observable
  c  a + the native moments at every save point (k_moments_tile, and k_moments_finish past 12 qubits)
  p  a + the rows as Z-string PauliObservables (S = the identity string, B_q = (1 - Z_q) / 2 ... as 1 + N + N(N-1)/2 one-string
     observables: what the Pauli route of the library offers for them; the rows are then <Z..Z>, from which the moments follow)
  d  a + the rows as diagonal tables (obs_diag), where the tables fit below 64 GiB
  f  forward + adjoint sweep with a dense random cotangent on every moments row at every save point
  g  forward + adjoint sweep with the same cotangent at the final save point only (every other save point: the zero path)
The per-save-point cost of a block is (leg - a) / (T + 1); of one dense injection (f - g) / T on top of the zero path.
mode "profile": three runs of c and of f and nothing else (the workload of a rocprofv3 --kernel-trace --stats run of its own, which
                gives the kernel times of k_moments_tile / k_moments_finish / k_moments_apply).
Floors: one read of the state (16 * 2^N bytes) for the forward block, one read plus one write for the cotangent, at the
bandwidth recorded in profiles/r04_bw_probe6.txt (READ_GBPS below).
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
from pulser_diff_amd.observables import PauliObservable, moment_rows  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, split_moments  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
T = int(sys.argv[2]) if len(sys.argv) > 2 else 8
mode = sys.argv[3] if len(sys.argv) > 3 else "time"
ROUNDS = 5
READ_GBPS = 5900.0  # profiles/r04_bw_probe6.txt: 67.1 MB moved in 11.4 us per launch at N = 20 (2R + 2W, launch gaps included), GB/s
dev = torch.device("cuda")
rows_grid = 4 if n % 4 == 0 else 1
coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows_grid) for j in range(n // rows_grid)], dtype=torch.float64)
iu = torch.triu_indices(n, n, 1)
u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev)
params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev, requires_grad=True)
seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
psi0[:, -1] = 1
ts = torch.arange(T + 1, dtype=torch.float64) / 1000
mask = (1 << n) - 1
n_rows = moment_rows(n)
pairs = [(q, r) for q in range(n) for r in range(q + 1, n)]
pauli = ([PauliObservable(n, [(1.0, {})])] + [PauliObservable(n, [(1.0, {q: "Z"})]) for q in range(n)]
         + [PauliObservable(n, [(1.0, {q: "Z", r: "Z"})]) for q, r in pairs])
table_bytes = n_rows * 8 * 2**n
tables = None
if table_bytes < 64 * 2**30:
    y = torch.arange(2**n, device=dev)
    bit = [((y >> (n - 1 - q)) & 1).to(torch.float64) for q in range(n)]
    tables = torch.stack([torch.ones(2**n, dtype=torch.float64, device=dev)] + bit + [bit[q] * bit[r] for q, r in pairs])
    del y, bit
cot = torch.randn(n_rows, T + 1, 1, generator=torch.Generator().manual_seed(0), dtype=torch.float64).to(dev)
cot_final = torch.zeros_like(cot)
cot_final[:, -1] = cot[:, -1]


def amp_det():
    amp = (0.5 * params[:4][seg])[None, None, :].contiguous()  # real: a drive without phase
    det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
    return amp, det


def spec_of(**kw):
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=False, **kw)


def forward(obs=None, **kw):
    with torch.no_grad():
        amp, det = amp_det()
        return evolve(amp, det, u, ts, psi0, spec_of(**kw), obs)[1]


def leg_grad(c):
    amp, det = amp_det()
    _, e = evolve(amp, det, u, ts, psi0, spec_of(moments=True), None)
    return torch.autograd.grad((c * e).sum(), params)[0]


LEGS = {"a": lambda: forward(), "c": lambda: forward(moments=True), "p": lambda: forward(pauli=pauli)}
if tables is not None:
    LEGS["d"] = lambda: forward(obs=tables)
LEGS["f"] = lambda: leg_grad(cot)
LEGS["g"] = lambda: leg_grad(cot_final)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


if mode == "profile":
    for _ in range(3):
        LEGS["c"]()
        LEGS["f"]()
    torch.cuda.synchronize()
    sys.exit(0)

reps = {}
for name, fn in LEGS.items():  # warm every shape, then size the windows
    fn()
    one = window(fn, 1)
    reps[name] = max(1, int(0.3 / max(one, 1e-6)) + 1)
# the three routes serve the same numbers: B_q = (S - <Z_q>) / 2 ... checked on the rows the routes share directly
mom = split_moments(LEGS["c"](), n)[1]
zz = LEGS["p"]()
assert (mom[0] - zz[0]).abs().max().item() < 1e-10 * mom[0].abs().max().item(), "S: native and Pauli rows disagree"
assert (mom[1:1 + n] - 0.5 * (zz[0] - zz[1:1 + n])).abs().max().item() < 1e-10 * mom[0].abs().max().item(), "B_q: native and Pauli rows disagree"
if tables is not None:
    assert (mom - LEGS["d"]()).abs().max().item() < 1e-10 * mom[0].abs().max().item(), "native and diagonal rows disagree"
times = {k: [] for k in LEGS}
for _ in range(ROUNDS):
    for name, fn in LEGS.items():
        times[name].append(window(fn, reps[name]))
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
state_bytes = 16 * 2**n
floor_read = state_bytes / (READ_GBPS * 1e9) * 1e6  # us
print(f"N={n} T={T} B=1 rows={n_rows}  ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
for k in LEGS:
    print(f"  leg {k:2s}: {med[k] * 1e3:10.3f} ms   spread {spread[k] * 100:5.1f} %   ({reps[k]} runs per window)")
per = lambda a, b, steps: (med[a] - med[b]) / steps * 1e6  # noqa: E731
c_us, p_us = per("c", "a", T + 1), per("p", "a", T + 1)
print(f"  forward block per save point: native {c_us:.2f} us   Pauli Z strings {p_us:.2f} us ({p_us / max(c_us, 1e-9):.1f} x)"
      + (f"   diagonal tables {per('d', 'a', T + 1):.2f} us ({table_bytes / 2**30:.2f} GiB of tables)" if tables is not None
         else f"   diagonal tables: not run ({table_bytes / 2**30:.1f} GiB of tables)"))
print(f"  floor of the forward block: one read of the state, {state_bytes / 2**20:.3f} MiB at {READ_GBPS:.0f} GB/s = {floor_read:.2f} us"
      f"  -> achieved {100 * floor_read / max(c_us, 1e-9):.1f} % of it (wall clock, launches included)")
inj_us = per("f", "g", T)
print(f"  dense cotangent injection per save point, on top of the zero path: {inj_us:.2f} us   (floor of the whole injection, one read"
      f" and one write: {2 * floor_read:.2f} us; the kernel's own time: mode \"profile\")")
