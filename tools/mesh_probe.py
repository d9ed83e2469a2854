"""GPU probe (not part of the suite): time of vrt_volume_extract_mesh on the device against the host pass, on the filled
voxelized_torus(8) (257^3 samples: config 3's volume), whole grid, iso 0.

Per run: the end-to-end call that fetches everything (a host clock around the synchronous call: count pass, scan, read-back of the
totals, emit pass, copy of the four arrays to the caller), the count-only call (all four pointers NULL: count pass, scan, read-back of
the totals), and the host converter (VVolumeConverter::ExtractMesh through vrh_extract_mesh: its count call and its fetch call, each of
which runs the whole pass) on the same field.  Medians over --reps calls after --warmup untimed ones (the first call grows the
scratch buffers).  The kernels' own time comes from a kernel trace of this probe, in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/mesh_probe.py --no-host: the rows mesh_count_kernel, run_scan_*_kernel and
mesh_emit_kernel).  count_pass_bytes_read is what the count pass has to read once, N^3 floats; over the count kernel's time it gives
the rate to hold against the HBM peak.  Prints one JSON line.

    python tools/mesh_probe.py [--reps 20] [--warmup 3] [--res 8] [--format f32|texel16] [--no-host]
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


def median_ms(fn, reps, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--format", choices=("f32", "texel16"), default="f32")
    ap.add_argument("--no-host", action="store_true", help="skip the host converter (for the kernel-trace run)")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 calls make the median")

    vol = workloads.voxelized_torus(args.res)
    vx.fill_enclosed_host(vol, 1.0, 1)
    vol.set_device_format(_abi.FORMAT_TEXEL16 if args.format == "texel16" else _abi.FORMAT_F32)
    N = vol.N
    out = {"workload": f"voxelized_torus({args.res}) after fill_enclosed: {N}^3 samples, {args.format}, whole grid, iso 0", "reps": args.reps,
           "warmup": args.warmup, "unit": "ms: median (and fastest) of the repetitions, host clock around the synchronous call"}
    with v.VHipRenderer() as r:
        r.upload_volume(0, vol)
        lib, ctx = r._lib, r._ctx
        res = _abi.vrt_mesh_result()

        def count_only():
            _abi.check(lib.vrt_volume_extract_mesh(ctx, 0, 0.0, None, None, None, None, None, 0, None, 0, C.byref(res)), "vrt_volume_extract_mesh")
            return int(res.vertices), int(res.quads)

        V, Q = count_only()
        pos, nrm = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
        mat, idx = np.zeros(V, np.uint8), np.zeros(6 * Q, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def fetch():
            _abi.check(lib.vrt_volume_extract_mesh(ctx, 0, 0.0, None, None, p(pos), p(nrm), p(mat), V, p(idx), 6 * Q, C.byref(res)), "vrt_volume_extract_mesh")

        out["vertices"], out["triangles"] = V, 2 * Q
        out["mesh_bytes_copied_out"] = int(pos.nbytes + nrm.nbytes + mat.nbytes + idx.nbytes)
        out["count_pass_bytes_read"] = N ** 3 * 4
        out["run_records_bytes"] = (N - 1) * (N - 1) * ((N - 1 + 63) // 64) * 16
        out["device_call"] = median_ms(fetch, args.reps, args.warmup)[:2]
        out["device_count_only"] = median_ms(count_only, args.reps, args.warmup)[:2]
        out["python_extract_mesh_count_then_fetch"] = median_ms(lambda: r.extract_mesh(0), args.reps, args.warmup)[:2]
    if not args.no_host:
        host = median_ms(lambda: vx.extract_mesh_host(vol, 0.0, texel16=False), 3, 1)
        out["host_extract_mesh_host_count_then_fetch"] = host[:2]
        out["host_vertices_triangles"] = [host[2][4]["vertices"], 2 * host[2][4]["quads"]]
        lib_h = vx.load_host()
        rec = np.zeros(N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        rec["density"], rec["material"] = np.asarray(vol.density, np.float32).reshape(-1), np.asarray(vol.material_id, np.uint8).reshape(-1)
        hres = _abi.vrt_mesh_result()
        one = lambda: lib_h.vrh_extract_mesh(rec.ctypes.data, N, float(vol.VolumeExtends), 0, 0.0, None, None, None, None, None, 0, None, 0, C.byref(hres))
        out["host_pass_alone"] = median_ms(one, 5, 1)[:2]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
