"""Cost of the native occupation correlations of a density-matrix register (profiles/dm_occupation_moments.txt):
    python tools/time_dm_moments.py [atoms ...]          (default: 6 9 12)

Shape: the doubled register of n atoms (2n qubits) under the c3 template of bench.py (one phase-free global drive of 4
piecewise-constant segments), T steps (100; 20 at 12 atoms, where one state is 268 MB), KRYLOV_SE, B = 1, no gradient,
store_states=False.  The rows are functionals of whatever vector is on the device, so no dissipator is needed to time them.  Legs,
alternated inside every round and timed with device events around whole forward runs:
  base   forward, no observable
  mom    base + the DmMoments block (1 + n + n(n-1)/2 rows, one k_dm_moments launch per chunk of save points)
  diag   base + as many of the same rows as fit RYDIFF_MAX_DM_DIAG = 64, handed over as dm_diag tables (k_dm_trace, one row per grid.z)
per save point: (leg - base) / (T + 1).  The two legs agree on the rows they share before they are timed.  Every shape is warmed; a
window holds enough repeats to last well above 0.2 s; the median of 5 rounds is reported with its spread."""
import gc
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

gc.collect()
gc.freeze()
from pulser_diff_amd.observables import MAX_DM_DIAG, DensityMatrixObservables, moment_rows  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve  # noqa: E402

ATOMS = [int(a) for a in sys.argv[1:]] or [6, 9, 12]
ROUNDS = 5
dev = torch.device("cuda")


def bit_tables(n, count):
    """The first `count` rows of the block as dm_diag tables: 1, x_q, x_q x_r; atom q is bit n-1-q of x."""
    x = torch.arange(2 ** n)
    bits = [((x >> (n - 1 - q)) & 1).to(torch.float64) for q in range(n)]
    rows = [torch.ones(2 ** n, dtype=torch.float64)] + bits + [bits[q] * bits[r] for q in range(n) for r in range(q + 1, n)]
    return torch.stack(rows[:count]).to(dev)


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / reps


for n in ATOMS:
    nq, T = 2 * n, (20 if n >= 12 else 100)
    side = 4 if nq % 4 == 0 else 2
    coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(side) for j in range(nq // side)], dtype=torch.float64)
    iu = torch.triu_indices(nq, nq, 1)
    u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev)
    params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev)
    seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
    amp = (0.5 * params[:4][seg])[None, None, :].contiguous()  # real: a drive without phase
    det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
    ts = torch.arange(T + 1, dtype=torch.float64) / 1000
    rho0 = torch.zeros(1, 4 ** n, dtype=torch.complex128, device=dev)
    rho0[:, -1] = 1
    mask = (1 << nq) - 1
    rows = moment_rows(n)
    n_diag = min(rows, MAX_DM_DIAG)
    tables = bit_tables(n, n_diag)

    def forward(dm=None):
        with torch.no_grad():
            spec = ProblemSpec(nq, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=False, dm=dm)
            return evolve(amp, det, u, ts, rho0, spec, None)[1]

    legs = {"base": lambda: forward(), "mom": lambda: forward(DensityMatrixObservables(n, moments=True)),
            "diag": lambda: forward(DensityMatrixObservables(n, diag=tables))}
    a, b = legs["mom"](), legs["diag"]()
    assert a.shape[0] == rows and b.shape[0] == n_diag
    assert float((a[:n_diag] - b).abs().max()) <= 1e-12 * float(a[0].abs().max()), "the block and the dm_diag rows disagree"
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
    print(f"n={n} atoms ({nq} qubits) T={T} B=1  ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
    for k in legs:
        print(f"  leg {k:5s}: {med[k] * 1e3:10.3f} ms   spread {spread[k] * 100:5.1f} %   ({reps[k]} runs per window)")
    per = lambda leg: (med[leg] - med["base"]) / (T + 1) * 1e6  # noqa: E731
    print(f"  per save point: the block ({rows} rows) {per('mom'):.2f} us; {n_diag} of its rows as dm_diag tables {per('diag'):.2f} us; "
          f"ratio diag / block {per('diag') / max(per('mom'), 1e-9):.2f}")
    del tables, rho0
    torch.cuda.empty_cache()
