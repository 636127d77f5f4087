"""What the Gram matrices cost on top of the tangent sweep (profiles/geometry.txt):
    python tools/time_geometry.py PARENT_LIB [SOLVER] [N ...]        (SOLVER: krylov | dp5; default krylov, N = 16 18 20)

PARENT_LIB is librydiff.so built from the parent commit: its rydiff_forward_tangent is the baseline leg, on the same inputs, in the
same process.  All legs drive the C ABI directly (one plan, one workspace, the same device buffers), so no Python of either commit
is in the timed region:
  parent    rydiff_forward_tangent of PARENT_LIB
  tangent   rydiff_forward_tangent of this tree (the sweep moved into a shared function: must cost the same)
  geometry  rydiff_forward_geometry of this tree with dexpect_out (the parent's outputs plus the Gram matrices)
Shape: the c3 template of bench.py (rectangular register, one global drive of 4 piecewise-constant segments, 101 samples of 1 ns),
5 evaluation times = 4 save intervals of 25 ns, one diagonal observable (sum Z), D = 4 directions (the four drive amplitudes).
Per shape: a warm call of every leg, then 7 rounds; in every round each leg runs one window of at least 0.2 s, the legs interleaved
so that drift hits them alike.  Reported: the median over the rounds, the spread (max - min) / median of the parent leg, the ratio
geometry / parent, and the ratio the traffic count predicts: the Gram read is (1 + D) vector reads per save point against
2 (1 + D) vector transfers per factor pass, i.e. 1 + n_tsave / (2 * total factor passes)."""
import ctypes
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from pulser_diff_amd import _native  # noqa: E402
from pulser_diff_amd.solver import ProblemSpec, SolverType, _Call, _ptr, _stream_ptr  # noqa: E402
from pulser_diff_amd.utils import total_magnetization_diag  # noqa: E402

args = sys.argv[1:]
parent_path = Path(args.pop(0)).resolve()
solver_name = args.pop(0) if args and args[0] in ("krylov", "dp5") else "krylov"
sizes = [int(a) for a in args] or [16, 18, 20]
solver = {"krylov": SolverType.KRYLOV_SE, "dp5": SolverType.DP5_SE}[solver_name]
T, D, N_SAVE = 100, 4, 5
dev = torch.device("cuda")


def bind(path):
    """The three functions the legs call, bound by hand: PARENT_LIB has no geometry exports."""
    L = ctypes.CDLL(str(path))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    prob, info, tang = ctypes.POINTER(_native.RydProblem), ctypes.POINTER(_native.RydPlanInfo), ctypes.POINTER(_native.RydTangent)
    L.rydiff_plan.argtypes, L.rydiff_plan.restype = [prob, i32, i32, vp, vp, info], i32
    L.rydiff_last_error.restype = ctypes.c_char_p
    L.rydiff_tangent_workspace_bytes.argtypes, L.rydiff_tangent_workspace_bytes.restype = [prob, info, i32], ctypes.c_size_t
    L.rydiff_forward_tangent.argtypes, L.rydiff_forward_tangent.restype = [prob, info, tang, vp, vp, vp, vp, ctypes.c_size_t, vp], i32
    if hasattr(L, "rydiff_forward_geometry"):
        L.rydiff_geometry_workspace_bytes.argtypes, L.rydiff_geometry_workspace_bytes.restype = [prob, info, i32], ctypes.c_size_t
        L.rydiff_forward_geometry.argtypes, L.rydiff_forward_geometry.restype = [prob, info, tang, vp, vp, vp, vp, vp, ctypes.c_size_t, vp], i32
    assert (L.rydiff_sizeof_problem(), L.rydiff_sizeof_tangent()) == (ctypes.sizeof(_native.RydProblem), ctypes.sizeof(_native.RydTangent))
    return L


parent, new = bind(parent_path), bind(_native._LIB_PATH)
assert not hasattr(parent, "rydiff_forward_geometry"), "PARENT_LIB already has the geometry exports: not the parent commit's library"


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for n in sizes:
    rows = 4 if n % 4 == 0 else (2 if n % 2 == 0 else 1)
    coords = torch.tensor([[8.0 * i, 8.0 * j] for i in range(rows) for j in range(n // rows)], dtype=torch.float64)
    iu = torch.triu_indices(n, n, 1)
    u = (5420158.53 / (coords[iu[0]] - coords[iu[1]]).norm(dim=1) ** 6).to(dev).contiguous()
    params = torch.tensor([3.5, 5.0, 2.0, 4.0, -1.0, 0.5, 1.5, -0.5], dtype=torch.float64, device=dev)
    seg = (torch.arange(T + 1, device=dev) * 4 // (T + 1)).clamp(max=3)
    amp = (0.5 * params[:4][seg])[None, None, :].to(torch.complex128).contiguous()
    det = (-0.5 * params[4:][seg])[None, None, :].contiguous()
    d_amp = torch.stack([0.5 * (seg == d).to(torch.complex128) for d in range(D)])[:, None, None, :].contiguous()
    psi0 = torch.zeros(1, 2**n, dtype=torch.complex128, device=dev)
    psi0[:, -1] = 1
    ts = (torch.arange(N_SAVE, dtype=torch.float64) * (T // (N_SAVE - 1)) / 1000).numpy()
    zdiag = total_magnetization_diag(n)[None].to(dev).contiguous()
    mask = (1 << n) - 1
    call = _Call(ProblemSpec(n, 0.001, T + 1, (mask,), (mask,), solver=solver, store_states=False), amp, det, u, ts, 1, zdiag)
    call.problem.kernel_variant = 0
    p = call.problem
    tg = _native.RydTangent()
    tg.n_dir, tg.d_amp = D, d_amp.data_ptr()
    expect = torch.empty(1, N_SAVE, 1, dtype=torch.float64, device=dev)
    dexpect = {k: torch.empty(D, 1, N_SAVE, 1, dtype=torch.float64, device=dev) for k in ("parent", "tangent", "geometry")}
    gram = torch.empty(N_SAVE, 1, 1 + D, 1 + D, dtype=torch.complex128, device=dev)
    stream = _stream_ptr(dev)
    scratch = torch.empty(_native.PLAN_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    info = _native.RydPlanInfo()
    assert new.rydiff_plan(ctypes.byref(p), 0, 0, _ptr(scratch), stream, ctypes.byref(info)) == 0, new.rydiff_last_error()
    need = new.rydiff_geometry_workspace_bytes(ctypes.byref(p), ctypes.byref(info), D)
    assert need >= parent.rydiff_tangent_workspace_bytes(ctypes.byref(p), ctypes.byref(info), D) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def leg_tangent(L, key):
        rc = L.rydiff_forward_tangent(ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), _ptr(psi0), _ptr(expect), _ptr(dexpect[key]),
                                      _ptr(ws), ws.numel(), stream)
        assert rc == 0, L.rydiff_last_error()

    def leg_geometry():
        rc = new.rydiff_forward_geometry(ctypes.byref(p), ctypes.byref(info), ctypes.byref(tg), _ptr(psi0), _ptr(expect),
                                         _ptr(dexpect["geometry"]), _ptr(gram), _ptr(ws), ws.numel(), stream)
        assert rc == 0, new.rydiff_last_error()

    legs = {"parent": lambda: leg_tangent(parent, "parent"), "tangent": lambda: leg_tangent(new, "tangent"), "geometry": leg_geometry}
    for fn in legs.values():  # warm; the three legs give the same rows
        fn()
    torch.cuda.synchronize()
    scale = float(dexpect["parent"].abs().max())
    for key in ("tangent", "geometry"):
        assert float((dexpect[key] - dexpect["parent"]).abs().max()) <= 1e-10 * scale, key
    reps = {k: max(1, int(0.2 / max(window(fn, 1), 1e-6)) + 1) for k, fn in legs.items()}
    runs = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            runs[k].append(window(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = (max(runs["parent"]) - min(runs["parent"])) / med["parent"]
    predicted = 1.0 + N_SAVE / (2.0 * info.total_factors)
    print(f"N={n:2d} {solver_name:6s} D={D} n_tsave={N_SAVE} factor passes {info.total_factors}:  parent {med['parent'] * 1e3:9.3f} ms "
          f"(spread {spread * 100:.1f}%)   tangent {med['tangent'] * 1e3:9.3f} ms   geometry {med['geometry'] * 1e3:9.3f} ms   "
          f"geometry / parent {med['geometry'] / med['parent']:.4f} (traffic predicts {predicted:.4f})   tangent / parent "
          f"{med['tangent'] / med['parent']:.4f}", flush=True)
    del ws, psi0, gram
    torch.cuda.empty_cache()
