"""Where do the waves of an AIS workgroup land?  KABC_ABLATE=64 makes every wave of
the half-generation kernel write its HW_ID into the debug records; this prints, for
the C3 launch, how consumers and producers share SIMDs.  The geometry is the one
KABC_AIS_WIDE names (default 0): 0 = four waves per 64-row workgroup (wave 0 consumes,
1-3 produce), 1 = the wide geometry, the library's 8 or 12 waves per 128-row workgroup
(kabc_ais_wide_shipped; waves 0, 1 consume, the others produce)."""
import collections
import os
import sys

os.environ["KABC_PROBES"] = "1"   # the library variant with the probes compiled in

os.environ["KABC_ABLATE"] = "64"
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

nt = 16
e = k.AisEnsemble(bench.build_model(k), 65536, seed=1).init()
e.advance(2, nt)
e.set_debug(nt)
e.advance(1, nt)
d = e.get_debug(nt)            # [N][nt][6]; rows 0..32767 = half 0
hw = d[0:32768:ROWS].reshape(-1, 6 * nt)[:, 0:NW].astype(np.uint32)     # [workgroup][wave]
simd = (hw >> 4) & 3
cu = (hw >> 8) & 15
se = (hw >> 13) & 7
wave_id = hw & 15
print("geometry", f"wide, {NW} waves" if WIDE else "existing", "workgroups", hw.shape[0])
print("SIMD of (" + ", ".join(f"wave{w}" for w in range(NW)) + "), most common patterns:")
for pat, n in collections.Counter(map(tuple, simd.tolist())).most_common(8):
    print("  ", pat, n)
for c in range(NCONS):
    print(f"wave{c} (consumer) SIMD histogram:", np.bincount(simd[:, c], minlength=4).tolist())
    print(f"HW wave slot ids of wave{c}:", np.bincount(wave_id[:, c], minlength=16).tolist())
# producers beside each consumer; workgroups whose consumers share a SIMD
beside = (simd[:, NCONS:, None] == simd[:, None, :NCONS]).sum(axis=1)          # [workgroup][consumer]
print("producers on a consumer's SIMD, histogram per consumer (0, 1, 2, 3+):",
      [np.bincount(np.minimum(beside[:, c], 3), minlength=4).tolist() for c in range(NCONS)])
if NCONS == 2:
    same = simd[:, 0] == simd[:, 1]
    nb = NW // 4 - 1                     # producers beside a consumer: the rest of its SIMD
    expected = ~same & (beside[:, 0] == nb) & (beside[:, 1] == nb)
    print("workgroups with both consumers on one SIMD:", int(same.sum()))
    print("workgroups with the placement the shares are made for (consumers on two SIMDs, {nb} producer(s) "
          "beside each):".format(nb=nb), int(expected.sum()), "of", hw.shape[0])
