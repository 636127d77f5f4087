"""Cost of the native energy rows (profiles/energy_observables.txt):
    python tools/time_energy.py                 every size below, one child process per size under its own `timeout`; the report
                                                goes to stdout and to profiles/energy_observables.txt; stops at the first failure
    python tools/time_energy.py N [T [KERNEL]]  one size; KERNEL = ProblemSpec.energy_kernel: 0 automatic, 1 direct, 2 LDS-tile (from 13 qubits:
                                                the driver runs 1 and 2, which is how the automatic choice was made)
    python tools/time_energy.py N T composed    legs a and p only: needs nothing of the energy block, so it also runs in a checkout of the
                                                parent commit (copy this file into its tools/), which is where leg p of the profile is timed

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments), T steps
(T + 1 = 101 evaluation times), KRYLOV_SE, B = 1, psi0 = all ground.  Legs, alternated inside every round:
  a   forward, no observable
  e1  a + the row E at every save point            e2  a + E and M2
  p   a + E composed the only way the parent commit has: one Pauli row per drive group and quadrature (here: sum_q X_q, one
      observable of N strings) plus the moments block (S, B_q, B_qr carry the detuning and the interaction part); the host-side
      combination is not timed
  h   forward + adjoint sweep, cotangent on one diagonal row at the final save point (the run the block is added to)
  f   h + a dense random cotangent on E and M2 at every save point       g   h + the same cotangent at the final save point only
Per save point: forward block (e - a) / (T + 1); the two cotangent passes (f - g) / T on top of the zero path.  Floors measured in the
same process: one read of the state (a torch sum over its 2^(N+1) doubles) and one read plus one write (a device copy)."""
import gc
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SIZES = (12, 16, 20, 24)
STEP_TIMEOUT = {12: 120, 16: 120, 20: 180, 24: 400}  # seconds per child

if len(sys.argv) == 1:  # the driver: never touches the GPU itself
    out = []
    for n, kernel in [(n, k) for n in SIZES for k in ((1,) if n < 13 else (1, 2))]:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT[n]), sys.executable, str(Path(__file__).resolve()), str(n), "100", str(kernel)],
                           capture_output=True, text=True)
        out.append(r.stdout)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            out.append(f"N={n} kernel {kernel}: exit status {r.returncode}; stopped here\n{r.stderr[-2000:]}\n")
            print(out[-1], end="", flush=True)
            break
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "energy_observables.txt").write_text("".join(out))
    sys.exit(0 if r.returncode == 0 else 1)

sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

gc.collect()
gc.freeze()
from pulser_diff_amd.observables import PauliObservable  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, split_moments  # noqa: E402

n = int(sys.argv[1])
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
COMPOSED = len(sys.argv) > 3 and sys.argv[3] == "composed"
KERNEL = 0 if COMPOSED or len(sys.argv) <= 3 else int(sys.argv[3])
if not COMPOSED:
    from pulser_diff_amd.solver import split_energy  # noqa: E402
ROUNDS = 5
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
sum_x = [PauliObservable(n, [(1.0, {q: "X"}) for q in range(n)])]
y = torch.arange(2**n, device=dev)
zdiag = sum((1.0 - 2.0 * ((y >> q) & 1).to(torch.float64)) for q in range(n))[None].contiguous()
del y
gen = torch.Generator().manual_seed(0)
cot = torch.randn(2, T + 1, 1, generator=gen, dtype=torch.float64).to(dev)
cot_final = torch.zeros_like(cot)
cot_final[:, -1] = cot[:, -1]


def tables():
    amp = (0.5 * params[:4][seg])[None, None, :].contiguous()  # real: a drive without phase; samples ARE the save points (dt = 1 ns)
    det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
    return amp, det


def spec_of(**kw):
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=False, **kw)


def forward(energy=0, **kw):
    with torch.no_grad():
        amp, det = tables()
        e = dict(energy_amp=amp, energy_det=det) if energy else {}
        if energy:
            kw.update(energy=energy, energy_kernel=KERNEL)
        return evolve(amp, det, u, ts, psi0, spec_of(**kw), None, **e)[1]


def grad(c):
    amp, det = tables()
    e = dict(energy_amp=amp, energy_det=det) if c is not None else {}
    _, rows = evolve(amp, det, u, ts, psi0, spec_of(**(dict(energy=2, energy_kernel=KERNEL) if c is not None else {})), zdiag, **e)
    rest, en = split_energy(rows, 2 if c is not None else 0)
    loss = rest[0, -1, 0] + ((c * en).sum() if c is not None else 0.0)
    return torch.autograd.grad(loss, params)[0]


LEGS = {"a": lambda: forward(), "e1": lambda: forward(1), "e2": lambda: forward(2), "p": lambda: forward(pauli=sum_x, moments=True),
        "h": lambda: grad(None), "f": lambda: grad(cot), "g": lambda: grad(cot_final)}
if COMPOSED:
    LEGS = {k: LEGS[k] for k in ("a", "p")}


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
    reps[name] = max(1, int(0.3 / max(window(fn, 1), 1e-6)) + 1)
if COMPOSED:
    times = {k: [] for k in LEGS}
    for _ in range(ROUNDS):
        for name, fn in LEGS.items():
            times[name].append(window(fn, reps[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"N={n} T={T} composed route only (legs a, p): a {med['a'] * 1e3:.3f} ms, p {med['p'] * 1e3:.3f} ms -> "
          f"{(med['p'] - med['a']) / (T + 1) * 1e6:.2f} us per save point (Pauli sum_q X_q + moments block)")
    sys.exit(0)
# the composed route serves the same number: E = c <sum X> + dcoef (N S - sum B_q) + sum U_qr (S - B_q - B_r + B_qr)
with torch.no_grad():
    amp, det = tables()
    rows_p = LEGS["p"]()
    rest, mom = split_moments(rows_p, n)
    S, Bq, Bqr = mom[0], mom[1:1 + n], mom[1 + n:]
    e_p = (amp[0, 0].real[:, None] * rest[0] + 2.0 * det[0, 0][:, None] * (n * S - Bq.sum(0))
           + (u[:, None, None] * (S[None] - Bq[iu[0]] - Bq[iu[1]] + Bqr)).sum(0))
    e_n = LEGS["e1"]()[0]
    assert float((e_p - e_n).abs().max()) < 1e-9 * max(1.0, float(e_n.abs().max())), "native E and the composed E disagree"
# floors, in this process: one read of the state; one read and one write
a_vec = torch.view_as_real(psi0.clone()).reshape(-1)
b_vec = torch.empty_like(a_vec)
read_s = min(window(lambda: a_vec.sum(), 50) for _ in range(5))
copy_s = min(window(lambda: b_vec.copy_(a_vec), 50) for _ in range(5))
times = {k: [] for k in LEGS}
for _ in range(ROUNDS):
    for name, fn in LEGS.items():
        times[name].append(window(fn, reps[name]))
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
print(f"N={n} T={T} ({T + 1} evaluation times) B=1  energy_kernel={KERNEL} ({('automatic', 'direct', 'LDS-tile')[KERNEL]})  ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
for k in LEGS:
    print(f"  leg {k:2s}: {med[k] * 1e3:10.3f} ms   spread {spread[k] * 100:5.1f} %   ({reps[k]} runs per window)")
per = lambda a, b, steps: (med[a] - med[b]) / steps * 1e6  # noqa: E731
e1, e2, p_us, cot_us = per("e1", "a", T + 1), per("e2", "a", T + 1), per("p", "a", T + 1), per("f", "g", T)
print(f"  floors measured here: one read of the state ({16 * 2**n / 2**20:.3f} MiB) {read_s * 1e6:.2f} us; one read + one write {copy_s * 1e6:.2f} us "
      "(torch kernels, launch included)")
print(f"  forward block per save point: E {e1:.2f} us = {e1 / (read_s * 1e6):.2f} reads;  E and M2 {e2:.2f} us = {e2 / (read_s * 1e6):.2f} reads")
print(f"  cotangent passes per save point (dense cotangent, on top of the zero path): {cot_us:.2f} us = {cot_us / (copy_s * 1e6):.2f} x (read + write)")
print(f"  share of a whole run: forward + {100 * (med['e2'] - med['a']) / med['a']:.1f} % (two rows), "
      f"forward + gradient + {100 * (med['f'] - med['h']) / med['h']:.1f} % (dense cotangent), + {100 * (med['g'] - med['h']) / med['h']:.1f} % (final time only)")
faster = "faster" if e1 < p_us else "NOT faster"
if e1 <= 0.0:  # the block's launches hide behind the host's launch queue: the difference of the two medians is noise around zero
    faster = "not resolved (the forward block hides behind the launches of the run)"
print(f"  E alone against the composed route (Pauli sum_q X_q + moments block; leg p timed in THIS checkout): native {e1:.2f} us, composed {p_us:.2f} us per save point: "
      f"the block is {faster}" + (f" ({p_us / e1:.2f} x)" if e1 > 0.0 else ""))
