"""Phase timeline of the ADJOINT BLOCK pass k_chain2_bwd (tuning builds with -DRYDIFF_TIMELINE only):
make -C pulser-diff_amd/csrc timeline && RYDIFF_LIB=pulser-diff_amd/csrc/librydiff_timeline.so python tools/timeline_pair_bwd.py
RYDIFF_VARIANT=20 / 21: tape vectors staged through registers / by LDS-DMA; 22..29: request order and store policy of the block
kernels; 32, 33: paced requests; 35: P_X x_b on the tape, with the x-round that rebuilds x_a ahead of round A (default: the
automatic choice).  "landed" is stamped by wave 0 once its own elements are back."""
import ctypes, os, runpy, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
sys.argv = ["time_fwdgrad.py", "20", "10"]
runpy.run_path(str(Path(__file__).resolve().parent / "time_fwdgrad.py"), run_name="__main__")
import torch
from pulser_diff_amd import _native
tiles = 256
# [4096][8] stamps, then [4][4096]: slots 8 (mu landed), 9 (w landed), 10 (x_a landed), 11 (variant 35: the x_b tile is published, the x-round starts)
buf = np.zeros(4096 * 12, dtype=np.uint64)
L = _native.lib()
L.rydiff_debug_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int]
assert L.rydiff_debug_timeline(buf.ctypes.data, buf.size) == 0
t = buf[:tiles * 8].reshape(tiles, 8).astype(np.int64)
mu = buf[4096 * 8:4096 * 8 + tiles].astype(np.int64) - t[:, 0]
wl = buf[4096 * 9:4096 * 9 + tiles].astype(np.int64) - t[:, 0]
xl = buf[4096 * 10:4096 * 10 + tiles].astype(np.int64) - t[:, 0]
xr = buf[4096 * 11:4096 * 11 + tiles].astype(np.int64) - t[:, 0]
rel = t - t[:, :1]
names = ["start", "loads landed", "round A done", "x_b consumed", "round B done", "mu_out stored", "w' stored", "t' stored"]
print(f"k_chain2_bwd, kernel variant {os.environ.get('RYDIFF_VARIANT', '0')}: cycles since the workgroup's own start, "
      "median [min .. max] over the 256 workgroups of the last launch that finishes one block and starts the next")
for k, nm in enumerate(names):
    print(f"{nm:14s} {np.median(rel[:, k]):8.0f} [{rel[:, k].min():6d} .. {rel[:, k].max():6d}]")
    if k == 0:
        print(f"{'mu landed':14s} {np.median(mu):8.0f} [{mu.min():6d} .. {mu.max():6d}]   (wave 0)")
        print(f"{'w landed':14s} {np.median(wl):8.0f} [{wl.min():6d} .. {wl.max():6d}]   (wave 0)")
        print(f"{'x_a landed':14s} {np.median(xl):8.0f} [{xl.min():6d} .. {xl.max():6d}]   (wave 0; paced: behind round A's barrier, the next line)")
        if buf[4096 * 11:4096 * 11 + tiles].any():  # (stamped by the kernel of variant 35 only; there "x_a landed" is: rebuilt)
            print(f"{'x-round starts':14s} {np.median(xr):8.0f} [{xr.min():6d} .. {xr.max():6d}]   (x_b landed and published; ahead of round A)")
own = int(rel[:, 7].max())
mhz = float(os.environ.get("RYDIFF_CLOCK_MHZ", "2400"))  # MI355X peak engine clock
print(f"in-kernel span (longest workgroup, start to last stamp): {own} cycles = {own / mhz:.2f} us at {mhz:.0f} MHz, a lower bound on the "
      "time (the clock under load is not above the peak clock); set it against the rocprofv3 duration of k_chain2_bwd")
