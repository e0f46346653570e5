"""Where do the waves of an AIS workgroup land?  KABC_ABLATE=64 makes every wave of
the half-generation kernel write its HW_ID into the debug records; this prints, for
the C3 launch, how consumers and producers share SIMDs.  The geometry is the one
KABC_AIS_WIDE names (default 0): 0 = four waves per 64-row workgroup (wave 0 consumes,
1-3 produce), 1 = the wide geometry, eight waves per 128-row workgroup (waves 0, 1
consume, 2-7 produce)."""
import collections
import os
import sys

os.environ["KABC_PROBES"] = "1"   # the library variant with the probes compiled in

os.environ["KABC_ABLATE"] = "64"
WIDE = os.environ.setdefault("KABC_AIS_WIDE", "0") != "0"   # (never the default rule: the layout follows it)
NW, ROWS, NCONS = (8, 128, 2) if WIDE else (4, 64, 1)       # waves and rows per workgroup, consumers
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import kissabc_jl_amd as k  # noqa: E402

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
print("geometry", "wide" if WIDE else "existing", "workgroups", hw.shape[0])
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
    expected = ~same & (beside[:, 0] == 1) & (beside[:, 1] == 1)
    print("workgroups with both consumers on one SIMD:", int(same.sum()))
    print("workgroups with the placement the shares are made for (consumers on two SIMDs, one producer "
          "beside each):", int(expected.sum()), "of", hw.shape[0])
