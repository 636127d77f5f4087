"""Phase timeline of the FORWARD BLOCK pass k_chain2 (tuning builds with -DRYDIFF_TIMELINE only):
make -C pulser-diff_amd/csrc timeline && RYDIFF_LIB=pulser-diff_amd/csrc/librydiff_timeline.so python tools/timeline_pair_fwd.py
RYDIFF_VARIANT=20, 22..29: request order and store policy of the block kernels; 31, 33, 34: paced requests (default: the automatic
choice).  "landed" is stamped by wave 0 once its own elements of the vector are back, "consumed" once it has used them.
The stamps are those of the last forward launch that finishes one block and starts the next (full tape: v_mid is stored too)."""
import ctypes, os, runpy, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
sys.argv = ["time_fwdgrad.py", "20", "10"]
g = runpy.run_path(str(Path(__file__).resolve().parent / "time_fwdgrad.py"), run_name="__main__")
import torch
g["evolve"](g["amp"], g["det"], g["u"], g["ts"], g["psi0"], g["spec"], g["zdiag"][None])  # forward alone: the last stamps are k_chain2's
torch.cuda.synchronize()
from pulser_diff_amd import _native
tiles = 256
buf = np.zeros(4096 * 11, dtype=np.uint64)  # [4096][8] stamps, then [3][4096]: slots 8 (w landed), 9 (t landed), 10 (adjoint only)
L = _native.lib()
L.rydiff_debug_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int]
assert L.rydiff_debug_timeline(buf.ctypes.data, buf.size) == 0
t = buf[:tiles * 8].reshape(tiles, 8).astype(np.int64)
rel = t - t[:, :1]
extra = {2: ("w landed", buf[4096 * 8:4096 * 8 + tiles].astype(np.int64) - t[:, 0]),  # printed in front of the slot they precede
         3: ("t landed", buf[4096 * 9:4096 * 9 + tiles].astype(np.int64) - t[:, 0])}
names = ["start", "v landed, past round A's barrier", "w consumed", "t consumed", "y stored", "w' stored", "t' stored",
         "end (stores acknowledged)"]
print(f"k_chain2, kernel variant {os.environ.get('RYDIFF_VARIANT', '0')}: cycles since the workgroup's own start, "
      "median [min .. max] over the 256 workgroups of the last launch that finishes one block and starts the next")
for k, nm in enumerate(names):
    if k in extra:
        print(f"{extra[k][0]:34s} {np.median(extra[k][1]):8.0f} [{extra[k][1].min():6d} .. {extra[k][1].max():6d}]")
    print(f"{nm:34s} {np.median(rel[:, k]):8.0f} [{rel[:, k].min():6d} .. {rel[:, k].max():6d}]")
own = int(rel[:, 7].max())
mhz = float(os.environ.get("RYDIFF_CLOCK_MHZ", "2400"))  # MI355X peak engine clock
print(f"in-kernel span (longest workgroup, start to end): {own} cycles = {own / mhz:.2f} us at {mhz:.0f} MHz, a lower bound on the "
      "time (the clock under load is not above the peak clock); set it against the rocprofv3 duration of k_chain2")
