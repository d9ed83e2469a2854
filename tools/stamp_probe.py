"""Probe of vrt_volume_stamp (not part of the suite): what the call costs on the device against the host route it replaces, and what
the rule is worth.  Prints one JSON line per part; profiles/stamp.txt keeps them.

Timing (needs the GPU).  A sphere SDF of 129^3 samples is stamped into the torus SDF of 257^3 samples, at an oblique placement (scale
1.3) and at the identity placement (the source's box in the destination's corner), for every pair of formats.  Medians over --reps
calls after --warmup untimed ones, a host clock around the synchronous call:
  device_replace   REPLACE: every sample inside the source is written, every call, so each call runs the kernel over the footprint AND
                   the derive pipeline (bricks, cell records, tables) over the written box.
  device_no_derive a hard SUBTRACT repeated: into an F32 destination max(d, -v) == d everywhere after the first (untimed) call, so the
                   kernel runs over the same footprint with all its taps and writes nothing, and nothing is derived — the whole call
                   (memset, launch, copy-back of the partial records, two synchronisations) without the derive pipeline, not the
                   kernel alone.  A TEXEL16 destination stores the texel below m, so samples near the carved surface are written
                   again and again (written_by_a_repeated_subtract) and their box is derived: there the figure is no such floor.
  derive           device_replace - device_no_derive: what the rebuild of the written box costs (REPLACE's stores are in it too);
                   for a TEXEL16 destination it understates it, for the reason above.
  host_route       what a caller had to do before, on the same box (the one REPLACE reports) and with the same arithmetic
                   (csrc/stamp_core.h): vrt_volume_download_region of the box into the host mirror, VVolumeConverter::Stamp (through
                   vrh_stamp) on the mirror, vrt_volume_update_voxels of the box; its three legs are listed separately.
The kernel's own time is to be read from a kernel trace of this probe in a run of its own.

Accuracy (no GPU: the numpy reference of the contract, tests/stamp_ref.py).  An analytic sphere SDF (33^3 samples, radius 10.4 cells)
is stamped by ADD (reach 4) into an empty 65^3 field (density 30 everywhere) at an oblique placement, at scales 0.5, 1 and 1.7.  Every
grid edge of the destination whose ends differ in sign gives a point of the zero crossing by linear interpolation; reported are the
largest and the mean distance of those points from the analytic sphere (radius 10.4 * scale about the placement's position), in cells
of the destination.

    python tools/stamp_probe.py [--reps 20] [--warmup 2] [--accuracy-only]
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
from volumetricraytracer_amd import voxelizer as vx  # noqa: E402

VOXEL = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])


def quat(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2.0
    return tuple(a * math.sin(h)) + (math.cos(h),)


def sphere_sdf(res, extent, centre, radius_cells):
    """A sphere of radius_cells cells about `centre` (grid coordinates xyz) as a true distance in object units, density_scale 1."""
    vol = v.VVoxelVolume(res, extent)
    i = np.arange(vol.N, dtype=np.float64)
    x, z, y = i[:, None, None], i[None, :, None], i[None, None, :]
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius_cells
    vol.density = (d * float(vol.CellSize)).astype(np.float32)
    vol.material_id = (vol.density <= 0).astype(np.uint8)
    return vol


def accuracy():
    import stamp_ref as S
    import volume_ref as R

    Ns, Nd, radius = 33, 65, 10.4
    src = sphere_sdf(5, 16.0, (16.0, 16.0, 16.0), radius)
    position = np.array([31.3, 32.6, 30.9])
    out = {"part": "accuracy", "source": "33^3 sphere SDF, radius 10.4 cells", "destination": "65^3, density 30 everywhere", "op": "ADD, reach 4",
           "placement": "centre (31.3, 32.6, 30.9), turned 37 degrees about (1, 2, 3)", "unit": "cells of the destination", "scales": {}}
    for scale in (0.5, 1.0, 1.7):
        dst = v.VVoxelVolume(6, 100.0)
        d, m = np.full((Nd,) * 3, 30.0, np.float32), np.zeros((Nd,) * 3, np.uint8)
        rec = v.stamp_from_placement(Ns, position, quat((1, 2, 3), 37.0), scale, _abi.STAMP_ADD, reach=4.0)
        res = S.apply(d, m, R.F32, dst.VolumeExtends, 1.0, src.density, src.material_id, R.F32, src.VolumeExtends, 1.0, rec)
        dist = []
        grid = np.indices((Nd,) * 3).astype(np.float64)  # [x, z, y] index order
        for axis in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, Nd - 1), slice(1, Nd)
            a, b = d[tuple(lo)].astype(np.float64), d[tuple(hi)].astype(np.float64)
            cross = (a <= 0) != (b <= 0)
            t = a[cross] / (a[cross] - b[cross])
            pts = [grid[k][tuple(lo)][cross] + (t if k == axis else 0.0) for k in range(3)]  # x, z, y
            r = np.sqrt((pts[0] - position[0]) ** 2 + (pts[2] - position[1]) ** 2 + (pts[1] - position[2]) ** 2)
            dist.append(np.abs(r - radius * scale))
        dist = np.concatenate(dist)
        out["scales"][str(scale)] = {"written": res["written"], "crossings": int(dist.size), "max": round(float(dist.max()), 4),
                                     "mean": round(float(dist.mean()), 4)}
    print(json.dumps(out))


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(times)), 3), round(float(np.min(times)), 3)]


def records_of(vol):
    rec = np.zeros(vol.N ** 3, VOXEL)
    rec["density"], rec["material"] = np.asarray(vol.density, np.float32).reshape(-1), np.asarray(vol.material_id, np.uint8).reshape(-1)
    return rec


def timing(reps, warmup):
    DST, SRC = 0, 1
    dst = v.torus_volume(8, 100.0, 55.0, 22.0)
    dst.material_id = (dst.density <= 0).astype(np.uint8)
    dst.step_max = 2.0 * dst.GetCellSize()  # the empty-space tables are live: the derive pipeline rebuilds both levels
    src = sphere_sdf(7, 60.0, (64.0, 64.0, 64.0), 40.4)
    placements = {"oblique, scale 1.3": ((128.4, 127.7, 129.1), quat((1, 2, 3), 37.0), 1.3), "identity": ((64.0, 64.0, 64.0), (0, 0, 0, 1), 1.0)}
    host = vx.load_host()
    with v.VHipRenderer() as r:
        lib, ctx = r._lib, r._ctx
        for fmt_name, dfmt, sfmt in (("f32 into f32", 0, 0), ("texel16 into f32", 0, 1), ("f32 into texel16", 1, 0), ("texel16 into texel16", 1, 1)):
            for name, (position, rotation, scale) in placements.items():
                r.upload_volume(DST, dst.set_device_format(dfmt))
                r.upload_volume(SRC, src.set_device_format(sfmt))
                res = _abi.vrt_brush_result()
                replace = v.stamp_from_placement(src.N, position, rotation, scale, _abi.STAMP_REPLACE, material=_abi.STAMP_MATERIAL_SOURCE)
                carve = v.stamp_from_placement(src.N, position, rotation, scale, _abi.STAMP_SUBTRACT, material=0)
                call = lambda rec: _abi.check(lib.vrt_volume_stamp(ctx, DST, SRC, C.byref(rec), C.byref(res)), "vrt_volume_stamp")
                out = {"part": "timing", "formats": fmt_name, "placement": name, "source": f"{src.N}^3", "destination": f"{dst.N}^3", "reps": reps,
                       "unit": "ms: median, fastest"}
                out["device_replace"] = median_ms(lambda: call(replace), reps, warmup)
                lo, hi, out["written"] = tuple(res.lo), tuple(res.hi), int(res.written)
                out["box"] = [list(lo), list(hi)]
                call(carve)
                out["carved_by_the_first_subtract"] = int(res.written)
                out["device_no_derive"] = median_ms(lambda: call(carve), reps, warmup)
                out["written_by_a_repeated_subtract"] = int(res.written)
                out["derive"] = [round(a - b, 3) for a, b in zip(out["device_replace"], out["device_no_derive"])]
                if dfmt == 0 and sfmt == 0:  # the host route holds decoded floats: it is the F32 route
                    mirror, source = records_of(dst), records_of(src)
                    origin = (C.c_int * 3)(*lo)
                    size = (C.c_int * 3)(*[h - l + 1 for l, h in zip(lo, hi)])
                    (x0, y0, z0), (x1, y1, z1) = lo, hi
                    cube = mirror.reshape(dst.N, dst.N, dst.N)
                    box = np.zeros((x1 - x0 + 1, z1 - z0 + 1, y1 - y0 + 1), VOXEL)
                    hres = _abi.vrt_brush_result()

                    def down():
                        _abi.check(lib.vrt_volume_download_region(ctx, DST, origin, size, box.ctypes.data_as(C.c_void_p)), "vrt_volume_download_region")
                        cube[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1] = box

                    def stamp():
                        assert host.vrh_stamp(mirror.ctypes.data, dst.N, float(dst.VolumeExtends), float(dst.density_scale), 0, source.ctypes.data, src.N,
                                              float(src.VolumeExtends), float(src.density_scale), 0, C.byref(replace), C.byref(hres)) == 0

                    def up():
                        box[...] = cube[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1]
                        _abi.check(lib.vrt_volume_update_voxels(ctx, DST, origin, size, box.ctypes.data_as(C.c_void_p)), "vrt_volume_update_voxels")

                    host_reps = max(3, reps // 4)
                    out["host_download_region"] = median_ms(down, host_reps, 1)
                    out["host_stamp"] = median_ms(stamp, host_reps, 1)
                    out["host_update_voxels"] = median_ms(up, host_reps, 1)
                    out["host_route"] = median_ms(lambda: (down(), stamp(), up()), host_reps, 1)
                    out["host_written"] = int(hres.written)
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
