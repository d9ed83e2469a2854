"""GPU probe (not part of the suite): wall time of the enclosed-cavity fill on the device (vrt_volume_fill_enclosed) against the host
round trip it replaces — vrt_volume_download plus vrt_volume_upload_voxels of the same volume, with NO host-side fill in between (any
flood fill on the host costs more, so the round trip is a lower bound of the alternative) — on the 256^3 bench volume
(workloads.config3_voxelized(8): 257^3 samples with the shell metric), in both device formats.

The two variants alternate call by call; ahead of each one the unfilled volume is uploaded again, outside the timed region, so every
fill meets the same shell.  The first round is not counted.  The timing block (--reps rounds, the median of each variant) is repeated
--blocks times: the spread of the round trip's medians over the blocks (max - min) is the run-to-run noise the fill's median is read
against.  Prints one JSON line.

    python tools/volume_fill_probe.py [--reps 5] [--blocks 5] [--formats f32,texel16]
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

FORMATS = {"f32": _abi.FORMAT_F32, "texel16": _abi.FORMAT_TEXEL16}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--formats", default="f32,texel16")
    args = ap.parse_args()
    out = {"workload": "config3_voxelized(8): 257^3 samples, shell metric (both empty-space table levels live)", "reps": args.reps,
           "blocks": args.blocks, "unit": "ms, median wall time around the call(s), one value per block", "wall": 1.0, "material": 1}
    with v.VHipRenderer() as r:
        lib, ctx = r._lib, r._ctx
        for name in args.formats.split(","):
            vol = workloads.config3_voxelized(8, 16, device_format=FORMATS[name]).volumes()[0]
            rec = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
            res = _abi.vrt_fill_result()

            def fill():
                _abi.check(lib.vrt_volume_fill_enclosed(ctx, 0, 1.0, 1, C.byref(res)), "vrt_volume_fill_enclosed")

            def round_trip():
                _abi.check(lib.vrt_volume_download(ctx, 0, rec.ctypes.data_as(C.c_void_p)), "vrt_volume_download")
                _abi.check(lib.vrt_volume_upload_voxels(ctx, 0, vol.Resolution, vol.VolumeExtends, rec.ctypes.data_as(C.c_void_p)),
                           "vrt_volume_upload_voxels")

            variants = {"fill": fill, "round_trip": round_trip}
            times = {k: [] for k in variants}
            for block in range(args.blocks):
                t = {k: [] for k in variants}
                for rep in range(args.reps + (1 if block == 0 else 0)):  # round 0 grows the buffers
                    for k, fn in variants.items():
                        r.upload_volume(0, vol)  # the unfilled shell again, untimed
                        t[k].append(timed(fn))
                for k in variants:
                    times[k].append(float(np.median(t[k][1:] if block == 0 else t[k])))
            med = lambda k: float(np.median(times[k]))
            rt = times["round_trip"]
            out[name] = {"fill": times["fill"], "round_trip": rt, "fill_median": med("fill"), "round_trip_median": med("round_trip"),
                         "round_trip_spread": max(rt) - min(rt), "no_slower": med("fill") <= med("round_trip") + (max(rt) - min(rt)),
                         "speedup": med("round_trip") / med("fill"), "filled_samples": int(res.filled), "device_rounds": int(res.sweeps),
                         "box_lo": list(res.lo), "box_hi": list(res.hi)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
