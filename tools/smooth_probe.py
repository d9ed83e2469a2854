"""Probe of vrt_volume_smooth (not part of the suite): what the rule is worth, and what the call costs on the device against the host
route it replaces.  Prints one JSON line per part; profiles/volume_smooth.txt keeps them.

Accuracy (no GPU: the numpy reference of the contract, tests/smooth_ref.py).  An analytic sphere SDF of 10.4 cells on 33^3 samples
gets uniform noise of +-0.3 cells per sample and is smoothed over the whole grid (a box region far larger than the grid with a tiny
falloff: weight = strength everywhere) at strength 0.5 for 1, 2, 4 and 8 iterations, once with rebound 0 and once with rebound 1.
Every grid edge whose ends differ in sign gives a point of the zero crossing by linear interpolation; reported are the RMS and the
mean of those points' radial error (distance from the centre minus 10.4), in cells, before and after.

Timing (needs the GPU).  The torus SDF of 257^3 samples (the benched one, empty-space tables live), a sphere region of 32 cells
radius centred on the torus's ring, strength 0.5, falloff 4, rebound 0, at 1, 4 and 16 iterations, in both formats.  Medians over
--reps calls, a host clock around the synchronous call; the volume is uploaded again (untimed) before every timed call, so that
every call does the same work:
  device            the whole call: gather, the passes, the apply kernel, the copy-back of the partial records, and the derive pipeline
                    (bricks, cell records, tables) over the written box.
  device_no_derive  the same record on a second slot of the same size and format that holds 0 everywhere: every kernel runs over the
                    same box (their work does not depend on the values), nothing is written, nothing is derived.
  derive            device - device_no_derive: what the rebuild of the written box costs (the apply kernel's stores are in it too).
  per_pass          (device_no_derive at 16 iterations - at 1 iteration) / 15.
  host_route        what a caller had to do before, on the same box (the one the device call reports) and with the same arithmetic
                    (csrc/smooth_core.h): vrt_volume_download_region of the box into the host mirror, VVolumeConverter::Smooth
                    (through vrh_smooth, one thread) on the mirror, vrt_volume_update_voxels of the box; F32 only, as the host
                    route holds decoded floats.  Its three legs are listed separately.

    python tools/smooth_probe.py [--reps 20] [--warmup 2] [--accuracy-only]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volumetricraytracer_amd as v  # noqa: E402
from volumetricraytracer_amd import _abi  # noqa: E402
from volumetricraytracer_amd import voxelizer as vx  # noqa: E402

VOXEL = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])


def accuracy():
    import smooth_ref as S

    N, radius, noise = 33, 10.4, 0.3
    f0 = S.noisy_sphere(N, radius, noise)
    rms, mean = S.crossing_errors(f0, radius)
    out = {"part": "accuracy", "field": "33^3 sphere SDF, radius 10.4 cells, uniform noise +-0.3 cells", "region": "whole grid", "strength": 0.5,
           "unit": "cells: RMS and mean radial error of the zero crossings on grid edges", "before": {"rms": round(rms, 4), "mean": round(mean, 4)},
           "after": {}}
    for rebound in (0.0, 1.0):
        for it in (1, 2, 4, 8):
            rec = v.smooth_record(_abi.BRUSH_BOX, ((N - 1) / 2.0,) * 3, (N, N, N), 0.0, strength=0.5, iterations=it, falloff=1e-3, rebound=rebound)
            region, f = S.relax(f0, rec)
            assert region.all()
            rms, mean = S.crossing_errors(f, radius)
            out["after"][f"rebound {rebound:g}, {it} iterations"] = {"rms": round(rms, 4), "mean": round(mean, 4)}
    print(json.dumps(out), flush=True)


def median_ms(fn, reps, warmup, before=None):
    times = []
    for n in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if n >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(times)), 3), round(float(np.min(times)), 3)]


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
    host = vx.load_host()
    with v.VHipRenderer() as r:
        lib, ctx = r._lib, r._ctx
        for fmt_name, fmt in (("f32", 0), ("texel16", 1)):
            r.upload_volume(FLAT, flat.set_device_format(fmt))
            no_derive = {}
            for it in (1, 4, 16):
                rec = v.smooth_record(_abi.BRUSH_SPHERE, centre, (0, 0, 0), 32.0, strength=0.5, iterations=it, falloff=4.0, rebound=0.0, material=1)
                res = _abi.vrt_brush_result()
                call = lambda slot: _abi.check(lib.vrt_volume_smooth(ctx, slot, C.byref(rec), C.byref(res)), "vrt_volume_smooth")
                upload = lambda: r.upload_volume(EDITED, dst.set_device_format(fmt))
                out = {"part": "timing", "format": fmt_name, "volume": f"{N}^3", "region": "sphere, radius 32 cells", "iterations": it, "reps": reps,
                       "unit": "ms: median, fastest"}
                out["device"] = median_ms(lambda: call(EDITED), reps, warmup, before=upload)
                lo, hi, out["written"] = tuple(res.lo), tuple(res.hi), int(res.written)
                out["box"] = [list(lo), list(hi)]
                out["device_no_derive"] = median_ms(lambda: call(FLAT), reps, warmup)
                out["written_on_the_flat_slot"] = int(res.written)
                out["derive"] = [round(a - b, 3) for a, b in zip(out["device"], out["device_no_derive"])]
                no_derive[it] = out["device_no_derive"][0]
                if it == 16:
                    out["per_pass"] = round((no_derive[16] - no_derive[1]) / 15.0, 4)
                if fmt == 0:
                    mirror = np.zeros(N ** 3, VOXEL)
                    mirror["density"], mirror["material"] = dst.density.reshape(-1), dst.material_id.reshape(-1)
                    origin = (C.c_int * 3)(*lo)
                    size = (C.c_int * 3)(*[h - l + 1 for l, h in zip(lo, hi)])
                    (x0, y0, z0), (x1, y1, z1) = lo, hi
                    cube = mirror.reshape(N, N, N)
                    box = np.zeros((x1 - x0 + 1, z1 - z0 + 1, y1 - y0 + 1), VOXEL)
                    hres = _abi.vrt_brush_result()

                    def down():
                        _abi.check(lib.vrt_volume_download_region(ctx, EDITED, origin, size, box.ctypes.data_as(C.c_void_p)), "vrt_volume_download_region")
                        cube[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1] = box

                    def smooth():
                        assert host.vrh_smooth(mirror.ctypes.data, N, float(dst.VolumeExtends), float(dst.density_scale), 0, C.byref(rec), C.byref(hres)) == 0

                    def up():
                        box[...] = cube[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1]
                        _abi.check(lib.vrt_volume_update_voxels(ctx, EDITED, origin, size, box.ctypes.data_as(C.c_void_p)), "vrt_volume_update_voxels")

                    host_reps = max(3, reps // 4)
                    upload()
                    out["host_download_region"] = median_ms(down, host_reps, 1)
                    out["host_smooth"] = median_ms(smooth, host_reps, 1, before=down)
                    out["host_written"] = int(hres.written)
                    out["host_update_voxels"] = median_ms(up, host_reps, 1)
                    out["host_route"] = median_ms(lambda: (down(), smooth(), up()), host_reps, 1, before=upload)
                    out["host_route_over_device"] = round(out["host_route"][0] / out["device"][0], 1)
                print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--accuracy-only", action="store_true", help="the part that needs no GPU")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 calls make the median")
    accuracy()
    if not args.accuracy_only:
        timing(args.reps, args.warmup)


if __name__ == "__main__":
    main()
