"""GPU probe (not part of the suite): wall time of CSG brushes evaluated on the device (vrt_volume_apply_brushes) against the in-place
region update (vrt_volume_update_region) of the same boxes with data prepared beforehand, on the 256^3 bench volume
(workloads.config3_voxelized(8)), in both device formats.

  one dab   one ADD sphere whose footprint box (radius + reach + 2 samples either side) is 33^3 / 65^3 voxels, against one
            update of that box (ADD writes every sample within reach of the ball into the shell field's far background, so the
            written box, which the derived structures are rebuilt over, is the footprint less its 2-sample margin);
  a stroke  one call with 16 sphere records of radius 4 spaced 4 cells along x, against 16 updates of the 16 per-dab boxes.

The variants alternate call by call (every update puts the original voxels back, so every brush call edits the same field); the
first round is not counted.  The timing block (--reps rounds, the median of each variant) is repeated --blocks times: the spread of
the update's medians over the blocks is the run-to-run noise a brush median is read against.  Prints one JSON line.

    python tools/volume_brush_probe.py [--reps 20] [--blocks 5]
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

CENTRE = (200, 128, 128)  # on the torus surface
REACH = 2.0


def footprint(centre, radius, n):
    """The sample box a sphere record can write: radius + reach + 2 samples either side of an integer centre, clipped."""
    e = int(radius + REACH) + 2
    lo = [max(c - e, 0) for c in centre]
    hi = [min(c + e, n - 1) for c in centre]
    return lo, [h - l + 1 for l, h in zip(lo, hi)]


class Update:
    """vrt_volume_update_region of a box with the volume's own voxels, packed once."""

    def __init__(self, r, vol, lo, size):
        (x, y, z), (sx, sy, sz) = lo, size
        self.r, self.o, self.s = r, (C.c_int * 3)(*lo), (C.c_int * 3)(*size)
        self.d = np.ascontiguousarray(vol.density[x:x + sx, z:z + sz, y:y + sy])
        self.m = np.ascontiguousarray(vol.material_id[x:x + sx, z:z + sz, y:y + sy])

    def __call__(self):
        _abi.check(self.r._lib.vrt_volume_update_region(self.r._ctx, 0, self.o, self.s, self.d.ctypes.data_as(C.c_void_p),
                                                        self.m.ctypes.data_as(C.c_void_p)), "vrt_volume_update_region")


class Brushes:
    def __init__(self, r, recs):
        self.r, self.n, self.arr, self.res = r, len(recs), (_abi.vrt_brush * len(recs))(*recs), _abi.vrt_brush_result()

    def __call__(self):
        _abi.check(self.r._lib.vrt_volume_apply_brushes(self.r._ctx, 0, self.n, self.arr, C.byref(self.res)), "vrt_volume_apply_brushes")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    out = {"workload": "config3_voxelized(8): 257^3 samples, shell metric (both empty-space table levels live)", "reps": args.reps,
           "blocks": args.blocks, "unit": "ms, median wall time around the call(s), one value per block",
           "centre_xyz": CENTRE, "reach": REACH}
    with v.VHipRenderer() as r:
        for fmt, name in ((_abi.FORMAT_F32, "f32"), (_abi.FORMAT_TEXEL16, "texel16")):
            vol = workloads.config3_voxelized(8, 16, device_format=fmt).volumes()[0]
            r.upload_volume(0, vol)
            variants, written = {}, {}
            for label, radius in (("33^3", 12.0), ("65^3", 28.0)):
                variants[f"brush_{label}"] = Brushes(r, [v.sphere_brush(_abi.BRUSH_ADD, CENTRE, radius, 0.0, REACH, 1)])
                variants[f"update_{label}"] = Update(r, vol, *footprint(CENTRE, radius, vol.N))
            dabs = [(CENTRE[0] - 30 + 4 * i, CENTRE[1], CENTRE[2]) for i in range(16)]
            variants["stroke_brush_16_records"] = Brushes(r, [v.sphere_brush(_abi.BRUSH_ADD, c, 4.0, 0.0, REACH, 1) for c in dabs])
            updates = [Update(r, vol, *footprint(c, 4.0, vol.N)) for c in dabs]
            variants["stroke_update_16_calls"] = lambda: [u() for u in updates]
            times = {k: [] for k in variants}
            for block in range(args.blocks):
                t = {k: [] for k in variants}
                for rep in range(args.reps + (1 if block == 0 else 0)):  # round 0 grows the buffers
                    for k, fn in variants.items():
                        t[k].append(timed(fn))
                        if isinstance(fn, Brushes):
                            written[k] = int(fn.res.written)
                for k in variants:
                    times[k].append(float(np.median(t[k][1:] if block == 0 else t[k])))
            res = {k: times[k] for k in variants}
            res["written_samples"] = written
            med = lambda k: float(np.median(times[k]))
            for label in ("33^3", "65^3"):
                u = times[f"update_{label}"]
                res[f"dab_{label}"] = {"brush_median": med(f"brush_{label}"), "update_median": med(f"update_{label}"),
                                       "update_spread": max(u) - min(u),
                                       "no_slower": med(f"brush_{label}") <= med(f"update_{label}") + (max(u) - min(u))}
            res["stroke_speedup"] = med("stroke_update_16_calls") / med("stroke_brush_16_records")
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
