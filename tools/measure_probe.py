"""GPU probe (not part of the suite): what vrt_volume_measure costs, on voxelized_torus(8) (257^3 samples: config 3's volume) as the
Voxelizer leaves it — a shell — and on its filled, redistanced version (vrt_volume_fill_enclosed, then vrt_volume_redistance FROM_OUTSIDE
with a band of 8), whole grid, iso 0, in one process.

Three calls take turns, --rounds rounds: vrt_volume_measure; the count-only vrt_volume_extract_mesh (all four pointers NULL), which
reads the same N^3 floats once; and a full vrt_volume_download, which is what a caller had to do before there was a measure call (its
host loop over the N^3 records not included).  Per round and call: the median and the fastest of --reps synchronous calls after --warmup
untimed ones, host clock.  Prints one JSON line per volume.

    python tools/measure_probe.py [--rounds 3] [--reps 20] [--warmup 3] [--res 8]
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


def timed_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(times)), 4), round(float(np.min(times)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=8)
    args = ap.parse_args()

    vol = workloads.voxelized_torus(args.res)
    N = vol.N
    with v.VHipRenderer() as r:
        r.upload_volume(0, vol)
        lib, ctx = r._lib, r._ctx
        mesh, record = _abi.vrt_mesh_result(), np.zeros(N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        calls = {
            "measure": lambda: r.measure(0),
            "mesh_count_only": lambda: _abi.check(lib.vrt_volume_extract_mesh(ctx, 0, 0.0, None, None, None, None, None, 0, None, 0, C.byref(mesh)),
                                                  "vrt_volume_extract_mesh"),
            "download": lambda: _abi.check(lib.vrt_volume_download(ctx, 0, record.ctypes.data_as(C.c_void_p)), "vrt_volume_download"),
        }
        for name in ("shell", "filled and redistanced"):
            if name != "shell":
                r.fill_enclosed(0, None, 1.0, 1)
                r.redistance(0, None, 8, _abi.REDISTANCE_FROM_OUTSIDE)
            m = r.measure(0)
            p = _abi.mass_properties(m, args.res, vol.VolumeExtends)
            out = {"volume": f"voxelized_torus({args.res}), {name}: {N}^3 samples, f32, whole grid, iso 0", "reps": args.reps, "warmup": args.warmup,
                   "unit": "ms: [median, fastest] of the repetitions, host clock around the synchronous call",
                   "bytes_read_once": N ** 3 * 4, "download_bytes": N ** 3 * 8, "solid_samples": m["solid_samples"], "subsamples": m["subsamples"],
                   "active_cells": m["active_cells"], "quads": m["quads"], "object_volume": p["volume"], "object_area": p["area"]}
            for k in range(args.rounds):
                for call, fn in calls.items():
                    out[f"round {k + 1} {call}"] = timed_ms(fn, args.reps, args.warmup)
            print(json.dumps(out))


if __name__ == "__main__":
    main()
