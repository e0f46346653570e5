"""How long does each wave of an AIS batch wait at the workgroup barriers?
KABC_ABLATE=128: every wave writes (lifetime, time inside __syncthreads) in s_memtime
ticks (100 MHz) into the debug records; printed as means over the workgroups of the
C3 launch per wave.  The geometry is the one KABC_AIS_WIDE names (default 0): 0 = four
waves per 64-row workgroup (wave 0 consumes, 1-3 produce), 1 = the wide geometry, the
library's 8 or 12 waves per 128-row workgroup (kabc_ais_wide_shipped; waves 0, 1 consume, the
others produce; the words sit behind two words per wave, the first of them placement_probe.py's)."""
import os
import sys

os.environ["KABC_PROBES"] = "1"   # the library variant with the probes compiled in

os.environ["KABC_ABLATE"] = "128"
WIDE = os.environ.setdefault("KABC_AIS_WIDE", "0") != "0"   # (never the default rule: the layout follows it)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes  # noqa: E402

import numpy as np  # noqa: E402

import bench  # noqa: E402
import kissabc_jl_amd as k  # noqa: E402
from kissabc_jl_amd import _lib  # noqa: E402

geom = (ctypes.c_int32 * 3)()
_lib.load().kabc_ais_wide_shipped(geom)   # (waves, chunk, n_c) of the wide kernel of the library in use
NW, ROWS, NCONS = (geom[0], 128, 2) if WIDE else (4, 64, 1)   # waves and rows per workgroup, consumers

nt = int(os.environ.get("KABC_NT", "16"))
e = k.AisEnsemble(bench.build_model(k), 65536, seed=1).init()
e.advance(2, nt)
e.set_debug(nt)
e.advance(1, nt)
d = e.get_debug(nt).reshape(65536, -1)
t = d[0:32768:ROWS, 2 * NW:4 * NW].astype(np.float64).reshape(-1, NW, 2)   # [workgroup][wave][life, barrier]
print("geometry", f"wide, {NW} waves" if WIDE else "existing", "nt", nt, "ticks are s_memtime units")
for w in range(NW):
    life, bar = t[:, w, 0].mean(), t[:, w, 1].mean()
    print(f"wave {w} ({'consumer' if w < NCONS else 'producer'}): life {life:9.1f}  at barriers {bar:9.1f}  = {100 * bar / life:5.1f} %")
