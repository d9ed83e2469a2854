"""Probe of vrt_volume_warp (not part of the suite): what the rule is worth, and what the call costs on the device next to one plain
iteration of vrt_volume_smooth on the same region — existing code, in the same run, on the same box: the yardstick.  Prints one JSON
line per part; profiles/volume_warp.txt keeps them.

Accuracy (no GPU: the numpy reference of the contract, tests/warp_ref.py).  An analytic sphere SDF of 8 cells on 33^3 samples inside a
ball region of 14 cells at falloff 2 and strength 1 is grabbed, scaled and inflated; every grid edge whose ends differ in sign gives a
point of the zero crossing by linear interpolation; reported are the RMS and the mean of those points' radial error against the
analytic moved sphere, in cells.

Timing (needs the GPU).  The torus SDF of 257^3 samples (the benched one, empty-space tables live), a ball region of 40 cells radius
centred on the torus's ring, falloff 10, strength 1, material ids kept, in both formats: a fractional grab, a twist of 0.4 rad about
the region's centre, and an inflate by 1.5 cells — and vrt_volume_smooth with one plain iteration at strength 0.5 on the same ball.
Median, fastest and slowest of --reps calls, a host clock around the synchronous call (it ends in the read of the edit report, a
stream synchronise); the volume is uploaded again (untimed) before every timed call, so that every call does the same work:
  device            the whole call: its kernels, the copy-back of the partial records, and the derive pipeline (bricks, cell records,
                    tables) over the written box.
  device_no_derive  the same record on a second slot of the same size and format that holds 0 everywhere: every kernel runs over the
                    same box (their work does not depend on the values); a grab, a twist and the smooth write nothing there and
                    derive nothing.  (The inflate writes -w * off there: its figure on this slot includes the derive.)
  derive            device - device_no_derive.

    python tools/warp_probe.py [--reps 20] [--warmup 3] [--accuracy-only]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volumetricraytracer_amd as v  # noqa: E402
from volumetricraytracer_amd import _abi  # noqa: E402


def accuracy():
    import warp_ref as W

    out = {"part": "accuracy", "field": "33^3 sphere SDF, radius 8 cells", "region": "ball of 14 cells, falloff 2, strength 1",
           "unit": "cells: RMS and mean radial error of the zero crossings on grid edges against the analytic moved sphere", "after": {}}
    for name, (rms, mean) in W.worth(v.warp_record).items():
        out["after"][name] = {"rms": round(rms, 4), "mean": round(mean, 4)}
    print(json.dumps(out), flush=True)


def spread_ms(fn, reps, warmup, before=None):
    times = []
    for n in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if n >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(times)), 3), round(float(np.min(times)), 3), round(float(np.max(times)), 3)]


def timing(reps, warmup):
    EDITED, FLAT = 0, 1
    dst = v.torus_volume(8, 100.0, 55.0, 22.0)
    dst.material_id = (dst.density <= 0).astype(np.uint8)
    dst.step_max = 2.0 * dst.GetCellSize()  # the empty-space tables are live: the derive pipeline rebuilds both levels
    N = dst.N
    flat = v.VVoxelVolume(8, 100.0)
    flat.step_max = dst.step_max
    ring = 55.0 / float(dst.CellSize)
    centre = ((N - 1) / 2.0 + ring, (N - 1) / 2.0 + 0.3, (N - 1) / 2.0 - 0.4)
    region = dict(shape=_abi.BRUSH_SPHERE, a=centre, b=(0, 0, 0), radius=40.0)
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    twist = tuple(axis * math.sin(0.2)) + (math.cos(0.2),)
    warps = [("grab by (2.3, -1.1, 0.7)", dict(pull=v.warp_from_motion(centre, translation=(2.3, -1.1, 0.7))[0])),
             ("twist of 0.4 rad", dict(pull=v.warp_from_motion(centre, rotation=twist)[0])),
             ("inflate by 1.5", dict(inflate=1.5))]
    smooth = v.smooth_record(_abi.BRUSH_SPHERE, centre, (0, 0, 0), 40.0, strength=0.5, iterations=1, falloff=10.0, rebound=0.0, material=-1)
    with v.VHipRenderer() as r:
        lib, ctx = r._lib, r._ctx
        for fmt_name, fmt in (("f32", 0), ("texel16", 1)):
            r.upload_volume(FLAT, flat.set_device_format(fmt))
            upload = lambda: r.upload_volume(EDITED, dst.set_device_format(fmt))
            res = _abi.vrt_brush_result()
            calls = [(name, lambda slot, rec=v.warp_record(falloff=10.0, strength=1.0, material=_abi.WARP_MATERIAL_KEEP, **region, **fields):
                      _abi.check(lib.vrt_volume_warp(ctx, slot, C.byref(rec), C.byref(res)), "vrt_volume_warp")) for name, fields in warps]
            calls.append(("smooth, 1 plain iteration", lambda slot: _abi.check(lib.vrt_volume_smooth(ctx, slot, C.byref(smooth), C.byref(res)),
                                                                             "vrt_volume_smooth")))
            for name, call in calls:
                out = {"part": "timing", "format": fmt_name, "volume": f"{N}^3", "region": "ball, radius 40 cells, falloff 10", "call": name, "reps": reps,
                       "unit": "ms: median, fastest, slowest"}
                out["device"] = spread_ms(lambda: call(EDITED), reps, warmup, before=upload)
                out["written"], out["box"] = int(res.written), [list(res.lo), list(res.hi)]
                out["device_no_derive"] = spread_ms(lambda: call(FLAT), reps, warmup)
                out["written_on_the_flat_slot"] = int(res.written)
                if name.startswith("inflate"):
                    r.upload_volume(FLAT, flat.set_device_format(fmt))  # the inflate wrote there
                out["derive"] = round(out["device"][0] - out["device_no_derive"][0], 3)
                print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--accuracy-only", action="store_true", help="the part that needs no GPU")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5 calls make the median")
    accuracy()
    if not args.accuracy_only:
        timing(args.reps, args.warmup)


if __name__ == "__main__":
    main()
