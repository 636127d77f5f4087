"""Cost of the tangent sweep with the native XY exchange (profiles/xy_tangent.txt):
    python tools/time_xy_tangent.py [out.txt]          both sections below, printed (and written to out.txt)
    python tools/time_xy_tangent.py workload N         the workload of one `rocprofv3 --kernel-trace --stats` run (started by the above)

One problem per register size: a global drive with a phase, a detuning, a Hermitian exchange with couplings of both signs
(sum |J| about N rad/us), KRYLOV_SE, 101 evaluation times 1 ns apart, one diagonal observable, D = 4 directions.

1. Whole sweep, wall clock around work that ends in a device synchronise (every shape warmed, windows of at least 0.3 s, 5 rounds with
   the legs alternated inside every round, median and spread = (max - min) / median):
     8 atoms        native  = evolve_tangent on the exchange term (RYDIFF_TANGENT_XY, k_factor_tangent<4, false, true>), directions
                              d_amp and d_det — what the dense route can take;
                    native+ = the same with d_xy as well;
                    dense   = the same sweep on 28 dense pair terms (RYDIFF_TANGENT_PAIR_TERMS, k_factor_tangent<4, true>): the route
                              the emulator's all-times entry points take without xy_native=True, and the only one before this kernel.
     12, 16, 20     native+ against the loop of native reverse sweeps: one forward run with stored states and one adjoint sweep per
                    evaluation time (one-hot cotangent on the observable), which delivers the gradient w.r.t. every table entry and
                    coupling — the only route past 8 atoms before this kernel.  At 20 qubits the loop runs 5 of the 101 sweeps
                    (k = 0, 25, 50, 75, 100) and the figure is scaled by 101 / 5: said so on its line.
   The routes are checked against each other before anything is timed (1e-8 of the largest entry).
2. Kernel time per factor pass: `rocprofv3 --kernel-trace --stats`, a run of its own per register size (three sweeps per route and
   nothing else), averages over all dispatches."""
import csv
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pulser_diff_amd import _native  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve, evolve_tangent  # noqa: E402

ROUNDS = 5
T = 100
N_DIR = 4
SIZES = (8, 12, 16, 20)
dev = torch.device("cuda")


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(legs):
    reps = {}
    for name, fn in legs.items():
        fn()  # warm
        reps[name] = max(1, int(0.3 / max(window(fn, 1), 1e-6)) + 1)
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            times[name].append(window(fn, reps[name]))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), reps[k]) for k, v in times.items()}


class Problem:
    def __init__(self, n):
        self.n = n
        g = torch.Generator().manual_seed(3 + n)
        P = n * (n - 1) // 2
        t = torch.linspace(0, 1, T + 2, dtype=torch.float64)
        self.amp = (0.5 * 5.0 * torch.sin(np.pi * t) ** 2 * np.exp(-0.3j)).to(torch.complex128)[None, None, :].to(dev)
        self.det = (-0.5 * 4.0 * (2 * t - 1))[None, None, :].to(dev)
        self.ts = torch.arange(T + 1, dtype=torch.float64) * 0.001
        self.psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
        self.psi0[:, 5] = 1
        self.J = (16.0 / n * (2.0 * torch.rand(P, generator=g, dtype=torch.float64) - 1.0)).to(dev)  # 2 rad/us at 8 atoms
        self.u = torch.zeros(P, dtype=torch.float64, device=dev)
        self.obs = torch.linspace(-1, 1, 2**n, dtype=torch.float64, device=dev)[None]
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
        self.d_amp = torch.complex(rn(N_DIR, 1, 1, T + 2), rn(N_DIR, 1, 1, T + 2)).to(dev)
        self.d_det = rn(N_DIR, 1, 1, T + 2).to(dev)
        self.d_xy = rn(N_DIR, P).to(dev)
        self.mask = (1 << n) - 1

    def spec(self, route, **kw):
        if route == "dense":
            blocks = []
            pairs = [(a, b) for a in range(self.n) for b in range(a + 1, self.n)]
            for p, (a, b) in enumerate(pairs):
                blk = np.zeros((4, 4), dtype=np.complex128)
                blk[1, 2] = blk[2, 1] = float(self.J[p])
                blocks.append((a, b, blk))
            kw["pair_terms"] = tuple(blocks)
        else:
            kw["xy_mode"] = 1
        return ProblemSpec(self.n, 0.001, T + 2, (self.mask,), (self.mask,), solver=SolverType.KRYLOV_SE, store_states=False, **kw)

    def tangent(self, route, with_dxy=False):
        extra = dict(flags=_native.TANGENT_PAIR_TERMS) if route == "dense" else dict(xy_pairs=self.J, d_xy=self.d_xy if with_dxy else None)
        return evolve_tangent(self.amp, self.det, self.u, self.ts, self.psi0, self.spec(route), self.obs, d_amp=self.d_amp,
                              d_det=self.d_det, **extra)

    def adjoint_loop(self, ks):
        """Gradients of the observable at the evaluation times `ks` w.r.t. every table entry and coupling: (len(ks), ...) each."""
        a, d, J = (t.clone().requires_grad_(True) for t in (self.amp, self.det, self.J))
        spec = self.spec("native")
        _, e = evolve(a, d, self.u, self.ts, self.psi0, spec, self.obs, xy_pairs=J)
        self.stats = spec.options.get("_last_stats", {})
        out = []
        for k in ks:
            cot = torch.zeros_like(e)
            cot[0, k, 0] = 1.0
            out.append(torch.autograd.grad(e, (a, d, J), grad_outputs=cot, retain_graph=True))
        return out

    def check(self):
        """The routes compute the same thing: native against dense (8 atoms), native+ against the reverse sweep at two times."""
        _, full = self.tangent("native", True)
        scale = float(full.abs().max())
        if self.n <= 8:
            _, nat = self.tangent("native")
            _, den = self.tangent("dense")
            assert float((nat - den).abs().max()) <= 1e-8 * float(den.abs().max()), "native and dense sweeps disagree"
        ks = (T // 2, T)
        for k, (ga, gd, gj) in zip(ks, self.adjoint_loop(ks)):
            for dd in range(N_DIR):
                want = float((ga.conj() * self.d_amp[dd]).real.sum() + (gd * self.d_det[dd]).sum() + (gj * self.d_xy[dd]).sum())
                assert abs(float(full[dd, 0, k, 0]) - want) <= 1e-8 * scale, f"tangent and adjoint disagree at N={self.n} k={k} d={dd}"


def sweeps(lines):
    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"1. whole sweep: {T + 1} evaluation times, D = {N_DIR}, KRYLOV_SE, B = 1 ({ROUNDS} rounds, legs alternated; median, spread = (max - min) / median)")
    for n in SIZES:
        pr = Problem(n)
        pr.check()
        nf = pr.stats.get("total_factors")
        if n == 8:
            legs = {"native": lambda: pr.tangent("native"), "native+": lambda: pr.tangent("native", True), "dense": lambda: pr.tangent("dense")}
            scale, note = 1.0, ""
        else:
            ks = list(range(T + 1)) if n < 20 else [0, 25, 50, 75, 100]
            scale = (T + 1) / len(ks)
            note = "" if scale == 1.0 else f"   [loop: {len(ks)} of {T + 1} reverse sweeps run, figure scaled by {T + 1} / {len(ks)}]"
            legs = {"native+": lambda: pr.tangent("native", True), "loop": lambda ks=ks: pr.adjoint_loop(ks)}
        res = measure(legs)
        for k, (med, spread, reps) in res.items():
            f = scale if k == "loop" else 1.0
            per = f"   {med * 1e6 / nf:8.2f} us per factor pass, launches included" if (nf and k != "loop") else ""
            say(f"  N={n:2d} {k:8s}: {med * f * 1e3:11.3f} ms   spread {spread * 100:5.1f} %   ({reps} runs per window){per}{note if k == 'loop' else ''}")
        if n == 8:
            a, b, c = res["native"][0], res["native+"][0], res["dense"][0]
            say(f"  N= 8: dense / native = {c / a:.2f}; dense / native+ = {c / b:.2f}   (above 1: the native sweep is faster)   "
                f"[{nf} factors per sweep, degree {pr.stats.get('degree')}]")
        else:
            a, b = res["native+"][0], res["loop"][0] * scale
            say(f"  N={n:2d}: loop / native+ = {b / a:.1f}   [{nf} factors per sweep, degree {pr.stats.get('degree')}]")
        del pr
        torch.cuda.empty_cache()


def workload(n):
    pr = Problem(n)
    for _ in range(3):
        pr.tangent("native", True)
        if n <= 8:
            pr.tangent("dense")
    torch.cuda.synchronize()


def kernel_stats(directory: Path) -> dict:
    files = sorted(directory.rglob("*kernel_stats.csv"))
    if not files:
        raise RuntimeError(f"rocprofv3 left no kernel statistics under {directory}")
    with open(files[0], newline="") as fh:
        return {row["Name"]: (int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]), float(row["MaxNs"])) for row in csv.DictReader(fh)}


def kernels(lines, scratch_dir: Path) -> int:
    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("")
    say("2. kernel time per factor pass (rocprofv3 --kernel-trace --stats, one run per register size: three sweeps per route; microseconds)")
    for n in SIZES:
        with tempfile.TemporaryDirectory(dir=scratch_dir) as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
                   sys.executable, str(Path(__file__).resolve()), "workload", str(n)]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
            if run.returncode != 0:
                print(run.stdout[-4000:])
                return run.returncode or 1  # nothing more is started on the GPU after a failure
            stats = kernel_stats(Path(tmp))
        for name, (calls, avg, lo, hi) in sorted(stats.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            if "k_factor_tangent" in name:
                say(f"  N={n:2d} {name:60s} calls {calls:6d}  avg {avg / 1e3:9.2f}  min {lo / 1e3:9.2f}  max {hi / 1e3:9.2f}")
    return 0


def main() -> int:
    out_path = Path(sys.argv[1]).resolve() if len(sys.argv) > 1 else None
    scratch = out_path.parent if out_path else Path(tempfile.gettempdir())
    scratch.mkdir(parents=True, exist_ok=True)
    # the profiler runs first: their parent has not opened the GPU yet (each child is a fresh process with the device to itself)
    second = []
    rc = kernels(second, scratch)
    if rc:
        return rc
    first = []
    sweeps(first)
    if out_path:
        out_path.write_text("\n".join(first + second) + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "workload":
        workload(int(sys.argv[2]))
    else:
        sys.exit(main())
