"""GPU probe (not part of the suite): wall time of a full re-upload of the 256^3 bench volume (workloads.config3_voxelized(8))
against an in-place region update (vrt_volume_update_region) of boxes of 1^3, 8^3, 32^3 and 64^3 voxels, in both device formats.
Median of --reps calls of each, timed around the C-ABI call (which returns with the device work done).  Prints one JSON line.

    python tools/volume_edit_probe.py [--reps 20]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import volumetricraytracer_amd as v  # noqa: E402
from volumetricraytracer_amd import _abi  # noqa: E402
from volumetricraytracer_amd import workloads  # noqa: E402

BOXES = (1, 8, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    out = {"workload": "config3_voxelized(8): 257^3 samples, shell metric (both empty-space table levels live)", "reps": args.reps,
           "unit": "ms, median wall time around the call", "box_origin_xyz": "box centred on the torus surface at voxel (200, 128, 128)"}
    with v.VHipRenderer() as r:
        for fmt, name in ((_abi.FORMAT_F32, "f32"), (_abi.FORMAT_TEXEL16, "texel16")):
            vol = workloads.config3_voxelized(8, 16, device_format=fmt).volumes()[0]
            r.upload_volume(0, vol)
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r.upload_volume(0, vol)
                t.append(time.perf_counter() - t0)
            res = {"full_upload": float(np.median(t)) * 1e3}
            for b in BOXES:
                o = [min(max(c - b // 2, 0), vol.N - b) for c in (200, 128, 128)]
                d = np.ascontiguousarray(vol.density[o[0]:o[0] + b, o[2]:o[2] + b, o[1]:o[1] + b])
                m = np.ascontiguousarray(vol.material_id[o[0]:o[0] + b, o[2]:o[2] + b, o[1]:o[1] + b])
                oo, ss = (C.c_int * 3)(*o), (C.c_int * 3)(b, b, b)
                t = []
                for _ in range(args.reps + 1):  # the first call grows the staging / scratch buffers
                    t0 = time.perf_counter()
                    _abi.check(r._lib.vrt_volume_update_region(r._ctx, 0, oo, ss, d.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)),
                               "vrt_volume_update_region")
                    t.append(time.perf_counter() - t0)
                res[f"update_{b}^3"] = float(np.median(t[1:])) * 1e3
            res["full_over_update_32^3"] = res["full_upload"] / res["update_32^3"]
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
