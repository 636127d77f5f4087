"""All-times parameter sensitivities: one tangent sweep against the loop of one-hot reverse sweeps (profiles/tangent_sweep.txt):
    python tools/time_tangent.py N SOLVER        (SOLVER: krylov | dp5)

Shape: the c3 template of bench.py (rectangular register, one phase-free global drive of 4 piecewise-constant segments), n_t = 101
evaluation times, one diagonal observable (sum Z), D = 4 directions = the four drive-amplitude parameters.  Legs:
  fwd      one automatic rydiff_forward with the observable (no gradient)
  tangent  one rydiff_forward_tangent: values and d<O>(t_k)/d(theta_d) for all k and d
  loop     what the existing API needs for the same numbers: one differentiated forward run, then n_t backward calls with a
           one-hot-in-time cotangent (derivative.deriv_param's torch.autograd.grad(..., retain_graph=True))
fwd and tangent: median of 3 windows of at least 0.2 s after a warm run; loop: one warm backward call, then one full loop.
The two routes are compared before anything is timed (1e-8 relative to the largest entry).

The table of the profile is one process per shape, every one under its own time limit, chained so that trouble ends the chain:
    timeout -k 10 120 python tools/time_tangent.py 4 krylov && timeout -k 10 120 python tools/time_tangent.py 4 dp5 && \\
    timeout -k 10 120 python tools/time_tangent.py 10 krylov && ... && timeout -k 10 300 python tools/time_tangent.py 18 dp5"""
import gc
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

gc.collect()
gc.freeze()
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, evolve_tangent  # noqa: E402
from pulser_diff_amd.utils import total_magnetization_diag  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
solver = {"krylov": SolverType.KRYLOV_SE, "dp5": SolverType.DP5_SE}[sys.argv[2] if len(sys.argv) > 2 else "krylov"]
T, D = 100, 4
dev = torch.device("cuda")
rows = 4 if n % 4 == 0 else (2 if n % 2 == 0 else 1)
coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows) for j in range(n // rows)], dtype=torch.float64)
iu = torch.triu_indices(n, n, 1)
u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev)
params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev, requires_grad=True)
seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
psi0[:, -1] = 1
ts = torch.arange(T + 1, dtype=torch.float64) / 1000
mask = (1 << n) - 1
zdiag = total_magnetization_diag(n)[None].to(dev)
# d amp_table / d params[d]: 0.5 on segment d
d_amp = torch.stack([0.5 * (seg == d).to(torch.complex128) for d in range(D)])[:, None, None, :].contiguous()


def tables():
    amp = (0.5 * params[:4][seg])[None, None, :].contiguous()  # real: a drive without phase
    det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
    return amp, det


def spec():
    return ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=solver, store_states=False)


def leg_fwd():
    with torch.no_grad():
        amp, det = tables()
        return evolve(amp, det, u, ts, psi0, spec(), zdiag)[1]


def leg_tangent():
    with torch.no_grad():
        amp, det = tables()
        return evolve_tangent(amp.to(torch.complex128), det, u, ts, psi0, spec(), zdiag, d_amp=d_amp)[1]


def differentiated_run():
    amp, det = tables()
    return evolve(amp, det, u, ts, psi0, spec(), zdiag)[1][0, :, 0]


def one_hot_backward(f, k):
    cot = torch.zeros(T + 1, dtype=torch.float64, device=dev)
    cot[k] = 1.0
    return torch.autograd.grad(f, params, grad_outputs=cot, retain_graph=True)[0][:D]


def leg_loop():
    f = differentiated_run()
    return torch.stack([one_hot_backward(f, k) for k in range(T + 1)])  # (n_t, D)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


# the two routes give the same numbers (this also warms every shape)
loop = leg_loop()
tangent = leg_tangent()[:, 0, :, 0].T  # (n_t, D)
err = (tangent - loop).abs().max().item() / loop.abs().max().item()
assert err < 1e-8, f"tangent sweep and adjoint loop disagree: {err:.2e}"
del loop, tangent

med = {}
for name, fn in (("fwd", leg_fwd), ("tangent", leg_tangent)):
    fn()
    reps = max(1, int(0.2 / max(window(fn, 1), 1e-6)) + 1)
    med[name] = statistics.median(window(fn, reps) for _ in range(3))
f_warm = differentiated_run()
one_hot_backward(f_warm, T)
del f_warm
torch.cuda.synchronize()
t0 = time.perf_counter()
leg_loop()
torch.cuda.synchronize()
med["loop"] = time.perf_counter() - t0
name = "KRYLOV_SE" if solver == SolverType.KRYLOV_SE else "DP5_SE"
print(f"N={n:2d} {name:9s} n_t={T + 1} D={D}:  fwd {med['fwd'] * 1e3:9.3f} ms   tangent {med['tangent'] * 1e3:9.3f} ms   "
      f"adjoint loop {med['loop'] * 1e3:10.3f} ms   (tangent / fwd {med['tangent'] / med['fwd']:.2f}, loop / tangent "
      f"{med['loop'] / med['tangent']:.1f}; routes agree to {err:.1e})")
