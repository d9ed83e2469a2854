"""GPU probe (not part of the suite): time of vrt_volume_redistance on the device against the host pass it replaces, on the filled
voxelized_torus(8) (257^3 samples, FROM_OUTSIDE), at bands 3 and 8, over the whole grid and over a 33^3 box around a point of the
tube's surface.

Per case: the end-to-end call (wall clock around vrt_volume_redistance, which waits for its own work: the two surfel runs, the
distance pass, the read-back of the result record and the rebuild of the derived buffers over the box); the host converter
(VVolumeConverter::Redistance) on the same input; and, for the box, download + host + upload of the box, the round trip a caller
without the device pass would make (a lower bound: the host pass there sees the box without its surroundings, less work than a
correct pass over the box grown by band + 1).  The library launches on a stream of its own, so an event pair of the caller's cannot bracket its
kernels one by one: an event pair on the caller's stream spans the whole call on the device's clock (the call waits for its work), and
the kernels' own time comes from a kernel trace of this probe (rocprofv3 --kernel-trace --stats -- python tools/...: the rows
redist_surfel_kernel and redist_distance_kernel).  Ahead of each repetition the filled volume is uploaded again, untimed, so every
call meets the same field.  The first repetition is not counted (it grows the scratch buffers).  Prints one JSON line.

    python tools/volume_redistance_probe.py [--reps 5] [--res 8] [--no-host-whole]
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
from volumetricraytracer_amd import voxelizer as vx  # noqa: E402
from volumetricraytracer_amd import workloads  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--no-host-whole", action="store_true", help="skip the host converter on the whole grid (minutes at resolution 8)")
    args = ap.parse_args()
    import torch  # the event pair only

    vol = workloads.voxelized_torus(args.res)
    vx.fill_enclosed_host(vol, 1.0, 1)
    N = vol.N
    # a point of the tube's outer surface: the sample nearest the grid's centre row where the field changes sign along x
    row = vol.density[:, N // 2, N // 2]
    x = int(np.flatnonzero((row[:-1] > 0) != (row[1:] > 0))[-1])
    lo = tuple(int(np.clip(c - 16, 0, N - 33)) for c in (x, N // 2, N // 2))
    hi = tuple(a + 32 for a in lo)
    out = {"workload": f"voxelized_torus({args.res}) after fill_enclosed: {N}^3 samples, FROM_OUTSIDE", "reps": args.reps,
           "unit": "ms, median over the repetitions", "box": [lo, hi], "cases": {}}
    with v.VHipRenderer() as r:
        lib, ctx = r._lib, r._ctx
        for band in (3, 8):
            for name, box in (("whole grid", None), ("33^3 box", (lo, hi))):
                call_ms, event_ms, info = [], [], None
                for rep in range(args.reps + 1):
                    r.upload_volume(0, vol)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()  # on the caller's stream: the call's kernels start after e0 and have ended before e1 (the call waits)
                    ms, info = timed(lambda: r.redistance(0, None, band, _abi.REDISTANCE_FROM_OUTSIDE, *(box or (None, None))))
                    e1.record()
                    e1.synchronize()
                    if rep:
                        call_ms.append(ms)
                        event_ms.append(e0.elapsed_time(e1))
                rec = {"call": float(np.median(call_ms)), "device_ms_event_pair_around_call": float(np.median(event_ms)),
                       "kernels_device_ms": None,  # the redist_* rows of the kernel trace, see above
                       "surfels": info["surfels"],
                       "near": info["near"], "written": info["written"], "surfel_scratch_bytes": info["surfels"] * 24,
                       "table_scratch_bytes": 256 + 8 * ((N + 7) // 8) ** 3}
                if box or not args.no_host_whole:
                    host = v.VVoxelVolume(args.res, vol.VolumeExtends)
                    host.density, host.material_id, host.density_scale = vol.density.copy(), vol.material_id.copy(), vol.density_scale
                    rec["host_converter"], _ = timed(lambda: vx.redistance_host(host, band, _abi.REDISTANCE_FROM_OUTSIDE, *(box or (None, None))))
                if box:
                    def round_trip():
                        d, m = r.download_region(0, lo, hi)
                        part = v.VVoxelVolume(5, vol.VolumeExtends)  # the box's samples alone do not hold its surroundings: a lower bound
                        part.density, part.material_id, part.density_scale = np.ascontiguousarray(d), np.ascontiguousarray(m), vol.density_scale
                        vx.redistance_host(part, band, _abi.REDISTANCE_FROM_OUTSIDE, unit=np.float32(vol.GetCellSize()) / np.float32(vol.density_scale))
                        size = (C.c_int * 3)(33, 33, 33)
                        _abi.check(lib.vrt_volume_update_region(ctx, 0, (C.c_int * 3)(*lo), size, part.density.ctypes.data_as(C.c_void_p), None),
                                   "vrt_volume_update_region")
                    r.upload_volume(0, vol)
                    rec["download_host_upload_lower_bound"], _ = timed(round_trip)
                out["cases"][f"band {band}, {name}"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
