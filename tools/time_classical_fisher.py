"""What the classical Gram matrix costs per save point, next to the Gram matrix (profiles/classical_fisher.txt):
    python tools/time_classical_fisher.py [OUT]                 (OUT: default profiles/classical_fisher.txt)

For N = 12, 16, 20 qubits and D = 1, 4, 8 directions the tool starts one child process per shape under
`rocprofv3 --kernel-trace --stats` (a run of its own per shape: the kernel names do not carry N) and reads the kernel times of
    k_tangent_cfi<D> + k_cfi_finish       the two launches of the classical Gram matrix (fisher_kernels.hpp)
    k_tangent_gram<D> + k_gram_finish     the two launches of the Gram matrix (gram_kernels.hpp): existing code, the yardstick — it
                                          reads the same (1 + D) 2^N 16 bytes
from the same run.  The child (`workload N D`) drives rydiff_forward_fisher through the C ABI with gram_out and cgram_out: the c3
template of bench.py (rectangular register, one global drive of 4 piecewise-constant segments, 101 samples of 1 ns, KRYLOV_SE),
B = 1, a seeded random normalised psi0 and D seeded random d_psi0 (generic amplitudes: no zeros, no special phases), 9 evaluation
times; one warm call, then 4 calls, so every kernel has 45 dispatches.  Reported per shape: the mean and the smallest kernel time of
each launch pair per save point (kernel times: the gaps between launches are not in them), their ratio, and the time one read of
(1 + D) 2^N 16 bytes takes at the HBM peak of 8.0 TB/s and at the 6.29 TB/s a float4 copy reaches on this part."""
import csv
import ctypes
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SIZES, WIDTHS = (12, 16, 20), (1, 4, 8)
N_SAVE, T, CALLS = 9, 100, 4
PEAK_TBPS, COPY_TBPS = 8.0, 6.29


def workload(n: int, n_dir: int) -> None:
    sys.path.insert(0, str(ROOT))
    import torch

    from pulser_diff_amd import _native
    from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, _ptr, _stream_ptr

    dev = torch.device("cuda")
    L = _native.lib()
    rows = 4 if n % 4 == 0 else (2 if n % 2 == 0 else 1)
    coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows) for j in range(n // rows)], dtype=torch.float64)
    iu = torch.triu_indices(n, n, 1)
    u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev).contiguous()
    params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev)
    seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
    amp = (0.5 * params[:4][seg])[None, None, :].to(torch.complex128).contiguous()
    det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
    gen = torch.Generator().manual_seed(1000 * n + n_dir)
    psi0 = torch.randn(1, 2**n, generator=gen, dtype=torch.complex128)
    psi0 = (psi0 / psi0.norm()).to(dev)
    d_psi0 = (torch.randn(n_dir, 1, 2**n, generator=gen, dtype=torch.complex128) / 2 ** (n / 2)).to(dev)
    ts = (torch.arange(N_SAVE, dtype=torch.float64) * (T // (N_SAVE - 1)) / 1000).numpy()
    mask = (1 << n) - 1
    call = _Call(ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=SolverType.KRYLOV_SE, store_states=False), amp, det, u, ts, 1, None)
    call.problem.kernel_variant = 0
    p = call.problem
    tg = _native.RydTangent()
    tg.n_dir, tg.d_psi0 = n_dir, d_psi0.data_ptr()
    gram = torch.empty(N_SAVE, 1, 1 + n_dir, 1 + n_dir, dtype=torch.complex128, device=dev)
    cgram = torch.empty(N_SAVE, 1, 1 + n_dir, 1 + n_dir, dtype=torch.float64, device=dev)
    stream = _stream_ptr(dev)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    info = _native.RydPlanInfo()
    _native.check(L.rydiff_plan(ctypes.byref(p), 0, 0, _ptr(scratch), stream, ctypes.byref(info)))
    need = L.rydiff_fisher_workspace_bytes_flags(ctypes.byref(p), ctypes.byref(info), n_dir, 0)
    assert need > 0, _native.last_error()
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for _ in range(1 + CALLS):
        _native.check(L.rydiff_forward_fisher(ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), _ptr(psi0), None, None, _ptr(gram),
                                              _ptr(cgram), _ptr(ws), ws.numel(), stream))
    torch.cuda.synchronize()
    # the two matrices agree where they must: C_00 = G_00
    assert float((cgram[:, 0, 0, 0] - gram[:, 0, 0, 0].real).abs().max()) <= 1e-12
    assert bool(torch.isfinite(cgram).all())


def kernel_times(directory: Path) -> dict:
    """{kernel name: (calls, mean ns, min ns)} from the kernel statistics of one rocprofv3 run."""
    files = sorted(directory.rglob("*kernel_stats.csv"))
    if not files:
        raise RuntimeError(f"rocprofv3 left no kernel statistics under {directory}")
    out = {}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]))
    return out


def pair(stats: dict, main: str, finish: str) -> tuple:
    """(mean us, min us) of the launch pair per save point: the templated kernel (its only instantiation in the run) plus the finish."""
    hit = [v for k, v in stats.items() if k.startswith(main) or f" {main}" in k]
    fin = [v for k, v in stats.items() if k.startswith(finish) or f" {finish}" in k]
    if len(hit) != 1 or len(fin) != 1:
        raise RuntimeError(f"expected one {main} and one {finish} in the kernel statistics, found {len(hit)} and {len(fin)}")
    expected = (1 + CALLS) * N_SAVE
    if hit[0][0] != expected or fin[0][0] != expected:
        raise RuntimeError(f"{main} / {finish}: {hit[0][0]} / {fin[0][0]} dispatches, expected {expected}")
    return (hit[0][1] + fin[0][1]) / 1e3, (hit[0][2] + fin[0][2]) / 1e3


def main() -> int:
    out_path = (Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "classical_fisher.txt").resolve()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    lines = [f"Classical Gram matrix (k_tangent_cfi<D> + k_cfi_finish) against the Gram matrix (k_tangent_gram<D> + k_gram_finish): kernel "
             f"time per save point,",
             f"rocprofv3 --kernel-trace --stats, one run per shape; B = 1, {N_SAVE} save points x {1 + CALLS} calls = "
             f"{(1 + CALLS) * N_SAVE} dispatches per kernel; mean (smallest) in us.",
             f"One read of (1 + D) 2^N 16 B at the HBM peak of {PEAK_TBPS} TB/s, and at the {COPY_TBPS} TB/s of a float4 copy.", ""]
    for n in SIZES:
        for d in WIDTHS:
            with tempfile.TemporaryDirectory(dir=out_path.parent) as tmp:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
                       sys.executable, str(Path(__file__).resolve()), "workload", str(n), str(d)]
                run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
                if run.returncode != 0:
                    print(run.stdout[-4000:])
                    return run.returncode or 1  # nothing more is started on the GPU after a failure
                stats = kernel_times(Path(tmp))
            cfi, gram = pair(stats, "k_tangent_cfi", "k_cfi_finish"), pair(stats, "k_tangent_gram", "k_gram_finish")
            nbytes = (1 + d) * 2**n * 16
            line = (f"N={n:2d} D={d}  bytes {nbytes / 2**20:8.2f} MiB   cfi {cfi[0]:8.2f} ({cfi[1]:8.2f})   gram {gram[0]:8.2f} ({gram[1]:8.2f})   "
                    f"cfi / gram {cfi[0] / gram[0]:.3f} ({cfi[1] / gram[1]:.3f})   read at peak {nbytes / (PEAK_TBPS * 1e6):7.2f} us, "
                    f"at copy rate {nbytes / (COPY_TBPS * 1e6):7.2f} us")
            print(line, flush=True)
            lines.append(line)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "workload":
        workload(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main())
