"""Phase timeline of the ADJOINT BLOCK pass k_chain2_bwd (tuning builds with -DRYDIFF_TIMELINE only):
make -C pulser-diff_amd/csrc timeline && RYDIFF_LIB=pulser-diff_amd/csrc/librydiff_timeline.so python tools/timeline_pair_bwd.py
RYDIFF_VARIANT=20 / 21: tape vectors staged through registers / by LDS-DMA (default: the automatic choice)."""
import ctypes, os, runpy, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
sys.argv = ["time_fwdgrad.py", "20", "10"]
runpy.run_path(str(Path(__file__).resolve().parent / "time_fwdgrad.py"), run_name="__main__")
from pulser_diff_amd import _native
tiles = 256
buf = np.zeros(tiles * 8, dtype=np.uint64)
L = _native.lib()
L.rydiff_debug_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int]
assert L.rydiff_debug_timeline(buf.ctypes.data, buf.size) == 0
t = buf.reshape(tiles, 8).astype(np.int64)
rel = t - t[:, :1]
names = ["start", "loads landed", "round A done", "x_b consumed", "round B done", "mu_out stored", "w' stored", "t' stored"]
print(f"k_chain2_bwd, kernel variant {os.environ.get('RYDIFF_VARIANT', '0')}: cycles since the workgroup's own start, "
      "median [min .. max] over the 256 workgroups of the last launch that finishes one block and starts the next")
for k, nm in enumerate(names):
    print(f"{nm:14s} {np.median(rel[:, k]):8.0f} [{rel[:, k].min():6d} .. {rel[:, k].max():6d}]")
