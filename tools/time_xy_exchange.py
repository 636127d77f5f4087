"""Cost of the native XY exchange term (profiles/xy_exchange.txt):
    python tools/time_xy_exchange.py compare [native|dense|both]   8 atoms, 28 pairs, Hermitian exchange, KRYLOV_SE, T = 100 intervals
    python tools/time_xy_exchange.py passes [N ...]                time per factor pass at 9, 12, 16, 20 qubits
    python tools/time_xy_exchange.py plan                          degree and factor count of the 9-atom example
    python tools/time_xy_exchange.py profile N                     the workload of a rocprofv3 --kernel-trace --stats run of its own

compare: the same problem and tables on the exchange family (ProblemSpec.xy_mode = 1, k_factor_xy / k_factor_bwd_xy) and as 28 dense
pair terms forced onto the direct family (kernel_variant = 1, k_factor_direct + pair_apply) — the only like-for-like pair there is.
Legs, alternated inside every round: f = forward with stored states; g = forward + adjoint sweep for the table gradients (what the
dense route can deliver); x (native only) = g with dL/dJ as well.  "dense" uses nothing the exchange added, so the same file times
the parent commit from a checkout of it.
passes: wall clock per factor pass (launches included, the stream kept full: 2 intervals of a long save interval so that one run is
tens of factors), forward and forward + adjoint, for the exchange family and for the ising direct kernels (kernel_variant = 1) at
the same N, next to the time one read plus one write of the state takes at READ_GBPS.
profile: three forward + gradient runs of the `passes` problem at N on each family and nothing else; under
`rocprofv3 --kernel-trace --stats` the averages of k_factor_xy / k_factor_bwd_xy (and of the ising direct kernels) are the KERNEL
times per factor pass, free of launch gaps and of the recomputed forward passes that the wall-clock "adjoint" figure contains.
Every shape is warmed; a window is closed by a synchronise and lasts well above 0.2 s; 5 rounds, median and (max - min) / median."""
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pulser_diff_amd.solver import ProblemSpec, SolverType, evolve  # noqa: E402

ROUNDS = 5
READ_GBPS = 5900.0  # profiles/r04_bw_probe6.txt
dev = torch.device("cuda")
mode = sys.argv[1] if len(sys.argv) > 1 else "compare"


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
        fn()
        reps[name] = max(1, int(0.3 / max(window(fn, 1), 1e-6)) + 1)
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            times[name].append(window(fn, reps[name]))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), reps[k]) for k, v in times.items()}


def couplings(n, seed=3, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return scale * (2.0 * torch.rand(n * (n - 1) // 2, generator=g, dtype=torch.float64) - 1.0)


def tables(n_samples, phase=0.3):
    t = torch.linspace(0, 1, n_samples, dtype=torch.float64)
    amp = 0.5 * 5.0 * torch.sin(np.pi * t) ** 2 * np.exp(-1j * phase)
    det = -0.5 * 4.0 * (2 * t - 1)
    return amp.to(torch.complex128)[None, None, :].to(dev), det[None, None, :].to(dev)


def problem(n, T, dt=0.001):
    amp, det = tables(T + 2)
    ts = torch.arange(T + 1, dtype=torch.float64) * dt
    psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
    psi0[:, 5 % 2**n] = 1
    mask = (1 << n) - 1
    return amp, det, ts, psi0, mask


def compare(which):
    n, T = 8, 100
    amp, det, ts, psi0, mask = problem(n, T)
    J = couplings(n)
    u = torch.zeros(n * (n - 1) // 2, dtype=torch.float64, device=dev)
    blocks = []
    for p, (a, b) in enumerate((a, b) for a in range(n) for b in range(a + 1, n)):
        blk = np.zeros((4, 4), dtype=np.complex128)
        blk[1, 2] = blk[2, 1] = float(J[p])
        blocks.append((a, b, blk))

    def spec(route):
        kw = dict(xy_mode=1) if route == "native" else dict(pair_terms=tuple(blocks), kernel_variant=1)
        return ProblemSpec(n, 0.001, T + 2, (mask,), (mask,), solver=SolverType.KRYLOV_SE, **kw)

    def run(route, grad, with_j=False):
        a = amp.clone().requires_grad_(grad)
        d = det.clone().requires_grad_(grad)
        extra = {}
        if route == "native":
            extra["xy_pairs"] = J.to(dev).requires_grad_(with_j)
        sp = spec(route)
        with torch.set_grad_enabled(grad):
            states, _ = evolve(a, d, u, ts, psi0, sp, None, **extra)
            last_stats[route] = sp.options.get("_last_stats", {})
            if grad:
                (states[-1].abs() ** 2 * torch.linspace(-1, 1, 2**n, dtype=torch.float64, device=dev)).sum().backward()
        return states.detach(), (a.grad, d.grad) if grad else None

    routes = ["native", "dense"] if which == "both" else [which]
    last_stats = {}
    legs = {}
    for r in routes:
        legs[f"{r} f"] = lambda r=r: run(r, False)
        legs[f"{r} g"] = lambda r=r: run(r, True)
        if r == "native":
            legs["native x"] = lambda: run("native", True, True)
    if which == "both":  # the two routes compute the same thing
        (sa, ga), (sb, gb) = run("native", True), run("dense", True)
        assert float((sa - sb).abs().max()) < 1e-9, "states of the two routes disagree"
        assert float((ga[0] - gb[0]).abs().max()) < 1e-8 * float(gb[0].abs().max()), "gradients of the two routes disagree"
    res = measure(legs)
    print(f"compare: N={n} pairs={n * (n - 1) // 2} T={T} KRYLOV_SE Hermitian   ({ROUNDS} rounds; median ms, spread = (max - min) / median)")
    for k, (med, spread, reps) in res.items():
        print(f"  {k:9s}: {med * 1e3:9.3f} ms   spread {spread * 100:5.1f} %   ({reps} runs per window)")
    for r, st in last_stats.items():
        print(f"  plan, {r}: degree {st.get('degree')} factors {st.get('total_factors')} family {st.get('kernel_family')} {st.get('kernel_fwd')} / {st.get('kernel_bwd')}")


def passes(sizes, profile_only=False):
    if not profile_only:
        print(f"passes: wall clock per factor pass, launches included ({ROUNDS} rounds, median; spread in brackets); floor = one read + one write "
                  f"of the state at {READ_GBPS:.0f} GB/s")
    for n in sizes:
        T = 2
        amp, det, ts, psi0, mask = problem(n, T, dt=0.05)  # long save intervals: tens of factors per run
        P = n * (n - 1) // 2
        J = couplings(n, scale=4.0 / max(n, 1)).to(dev)
        g = torch.Generator().manual_seed(5)
        u_ising = (4.0 / n * torch.rand(P, generator=g, dtype=torch.float64)).to(dev)
        zero = torch.zeros(P, dtype=torch.float64, device=dev)
        specs = {"xy": ProblemSpec(n, 0.05, T + 2, (mask,), (mask,), solver=SolverType.KRYLOV_SE, xy_mode=1, store_states=False),
                 "ising": ProblemSpec(n, 0.05, T + 2, (mask,), (mask,), solver=SolverType.KRYLOV_SE, kernel_variant=1, store_states=False)}
        obs = torch.linspace(-1, 1, 2**n, dtype=torch.float64, device=dev)[None]

        def run(kind, grad):
            a = amp.clone().requires_grad_(grad)
            extra = {"xy_pairs": J.clone().requires_grad_(grad)} if kind == "xy" else {}
            with torch.set_grad_enabled(grad):
                _, e = evolve(a, det, zero if kind == "xy" else u_ising, ts, psi0, specs[kind], obs, **extra)
                if grad:
                    e[0, -1, 0].backward()

        if profile_only:
            for _ in range(3):
                run("xy", True)
                run("ising", True)
            torch.cuda.synchronize()
            st = {k: specs[k].options["_last_stats"] for k in specs}
            print(f"profile: N={n}: 3 forward + gradient runs per family; factors per forward run: xy {st['xy']['total_factors']} "
                  f"({st['xy']['kernel_fwd']} / {st['xy']['kernel_bwd']}, tape {st['xy']['tape']}), ising {st['ising']['total_factors']} "
                  f"({st['ising']['kernel_fwd']} / {st['ising']['kernel_bwd']}, tape {st['ising']['tape']})")
            continue
        legs = {f"{k} {leg}": (lambda k=k, gr=gr: run(k, gr)) for k in specs for leg, gr in (("f", False), ("g", True))}
        res = measure(legs)
        floor = 2 * 16 * 2**n / (READ_GBPS * 1e9) * 1e6
        for kind in specs:
            st = specs[kind].options["_last_stats"]
            nf = st["total_factors"]
            f_us = res[f"{kind} f"][0] / nf * 1e6
            b_us = (res[f"{kind} g"][0] - res[f"{kind} f"][0]) / nf * 1e6
            print(f"  N={n:2d} {kind:5s}: forward {f_us:8.2f} us [{res[f'{kind} f'][1] * 100:4.1f} %]   adjoint {b_us:8.2f} us [{res[f'{kind} g'][1] * 100:4.1f} %]"
                  f"   floor {floor:7.2f} us   ({nf} factors, degree {st['degree']}, {st['kernel_fwd']} / {st['kernel_bwd']}, tape {st['tape']})")


def plan():
    n, T = 9, 5
    amp, det, ts, psi0, mask = problem(n, T, dt=0.04)
    g = torch.Generator().manual_seed(2)
    coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(3) for j in range(3)], dtype=torch.float64)
    coords = coords + 0.4 * (2.0 * torch.rand(coords.shape, generator=g, dtype=torch.float64) - 1.0)
    field = torch.tensor([1.0, 0.3], dtype=torch.float64)  # the in-plane part of (0, 1, 0.3)
    iu = torch.triu_indices(n, n, 1)
    diff = coords[iu[0]] - coords[iu[1]]
    r = diff.norm(dim=1)
    J = 3700.0 * (1 - 3 * ((diff @ field) / (r * field.norm())) ** 2) / r**3
    spec = ProblemSpec(n, 0.04, T + 2, (mask,), (mask,), solver=SolverType.KRYLOV_SE, xy_mode=1)
    with torch.no_grad():
        evolve(amp, det, torch.zeros_like(J).to(dev), ts, psi0, spec, None, xy_pairs=J.to(dev))
    st = spec.options["_last_stats"]
    print(f"plan: 3 x 3 atoms at 8 um, field (0, 1, 0.3), C3 = 3700, {T} save intervals of 40 ns: sum |J| = {float(J.abs().sum()):.3f} rad/us, "
          f"spectral interval [{st['spectral'][0]:.3f}, {st['spectral'][1]:.3f}], degree {st['degree']}, factors {st['total_factors']}, rho {st['rho']:.3f}")


if mode == "compare":
    compare(sys.argv[2] if len(sys.argv) > 2 else "both")
elif mode == "passes":
    passes([int(v) for v in sys.argv[2:]] or [9, 12, 16, 20])
elif mode == "profile":
    passes([int(sys.argv[2])], profile_only=True)
elif mode == "plan":
    plan()
else:
    raise SystemExit(__doc__)
