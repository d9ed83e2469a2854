"""GPU probe (not part of the suite): time of vrt_query_contacts against what a caller had before it, on the filled
voxelized_torus(8) (257^3 samples: config 3's volume) as A with a 65^3 sphere B resting on its highest surface point, one cell deep.

Per run, each a host clock around synchronous calls, medians over --reps calls after --warmup untimed ones:
  count            vrt_query_contacts with no output: the clip box, count pass, scan, read-back of the totals and the report
  fetch            the call that also returns the records (count pass again, emit pass, copy out)
  mesh_count_box   the count-only vrt_volume_extract_mesh of A over the samples of the same cell box (existing code: what the count
                   pass costs without B's gather), and mesh_count_grid over the whole grid
  composed         the chain a caller had: vrt_scene_set to B alone, vrt_volume_extract_mesh of A (count, then the positions; over the
                   same box: a caller who clips as well as the call does), the fp32 transform of every vertex in numpy,
                   vrt_query_points_host of all of them, the selection of distance <= margin, vrt_scene_set back; and composed_grid,
                   the same with the mesh of the whole grid
The kernels' own time comes from a kernel trace of this probe in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/contacts_probe.py: the rows contacts_*_kernel, mesh_*_kernel, points_kernel).  Prints one JSON line; the composed path's contacts
are checked against the call's, bit for bit, before anything is timed.

    python tools/contacts_probe.py [--reps 20] [--warmup 3] [--margin-cells 0.5]
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

f32 = np.float32


def median_ms(fn, reps, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.median(times)), 4), round(float(np.min(times)), 4)], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin-cells", type=float, default=0.5)
    args = ap.parse_args()

    A = workloads.voxelized_torus(8)
    vx.fill_enclosed_host(A, 1.0, 1)
    N, ext = A.N, float(A.VolumeExtends)
    cell = 2.0 * ext / (N - 1)
    margin = float(f32(args.margin_cells * cell))
    B = v.VVoxelVolume(6, 0.25 * ext)
    rb = 0.65 * B.VolumeExtends
    B.fill(lambda X, Y, Z: (np.sqrt((X * X + Y * Y) + Z * Z) - f32(rb)).astype(f32))
    out = {"workload": f"A: voxelized_torus(8) after fill_enclosed, {N}^3, f32; B: a {B.N}^3 sphere of radius {rb:.3f} resting one cell deep on "
                       f"A's highest surface point; margin {args.margin_cells} cells of A", "reps": args.reps, "warmup": args.warmup,
           "unit": "ms: [median, fastest] of the repetitions, host clock around the synchronous calls"}
    with v.VHipRenderer() as r:
        r.upload_volume(0, A)
        r.upload_volume(1, B)
        lib, ctx = r._lib, r._ctx
        mres = _abi.vrt_mesh_result()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)

        def mesh(origin=None, size=None, fetch=True):
            o = (C.c_int * 3)(*origin) if origin is not None else None
            s = (C.c_int * 3)(*size) if size is not None else None
            _abi.check(lib.vrt_volume_extract_mesh(ctx, 0, 0.0, o, s, None, None, None, 0, None, 0, C.byref(mres)), "vrt_volume_extract_mesh")
            if not fetch:
                return int(mres.vertices)
            pos = np.zeros((int(mres.vertices), 3), f32)
            if len(pos):
                _abi.check(lib.vrt_volume_extract_mesh(ctx, 0, 0.0, o, s, ptr(pos), None, None, len(pos), None, 6 * int(mres.quads), C.byref(mres)),
                           "vrt_volume_extract_mesh")  # (the capacities are checked whether or not an array is asked for)
            return pos

        top = mesh()
        top = top[np.argmax(top[:, 1])]
        place_b = tuple(float(f32(x)) for x in (top[0], top[1] + rb - cell, top[2]))
        both = v.VScene(Objects=[v.VVoxelObject(Volume=A), v.VVoxelObject(Position=place_b, Volume=B)]).to_abi()
        alone = v.VScene(Objects=[v.VVoxelObject(Volume=A), v.VVoxelObject(Position=place_b, Volume=B)]).to_abi()
        alone.instances[0] = both.instances[1]
        alone.n_instances = 1
        set_scene = lambda s: _abi.check(lib.vrt_scene_set(ctx, C.byref(s)), "vrt_scene_set")
        set_scene(both)
        cres = _abi.vrt_contacts_result()

        def count():
            _abi.check(lib.vrt_query_contacts(ctx, 0, 1, margin, None, 0, C.byref(cres)), "vrt_query_contacts")
            return int(cres.contacts)

        n = count()
        rec = np.zeros(n, v.CONTACT_DTYPE)

        def fetch():
            _abi.check(lib.vrt_query_contacts(ctx, 0, 1, margin, ptr(rec), n, C.byref(cres)), "vrt_query_contacts")
            return rec

        # the cells B's box can reach, restated: B is unrotated and unscaled, so its box is an interval per axis of A's grid
        lo = [max(0, int(np.floor((place_b[a] - B.VolumeExtends + ext) / cell)) - 2) for a in range(3)]
        hi = [min(N - 2, int(np.ceil((place_b[a] + B.VolumeExtends + ext) / cell)) + 2) for a in range(3)]
        size = [h - l + 2 for l, h in zip(lo, hi)]  # cells lo..hi need samples lo..hi + 1

        def composed(origin, size):
            set_scene(alone)
            pos = mesh(origin, size)
            # step 2 of the rule in fp32, as a caller writes it (A sits at the origin, unrotated: O is the identity)
            w = np.stack([(((O[a, 0] * pos[:, 0] + O[a, 1] * pos[:, 1]) + O[a, 2] * pos[:, 2]) + place_a[a]).astype(f32) for a in range(3)], axis=1)
            pts = v.make_points(w)
            res = np.zeros(len(pts), v.POINT_RESULT_DTYPE)
            _abi.check(lib.vrt_query_points_host(ctx, 0, 0.0, len(pts), ptr(pts), ptr(res)), "vrt_query_points_host")
            keep = ((res["flags"] & _abi.POINT_SAMPLED) != 0) & (res["distance"] <= f32(margin))
            set_scene(both)
            return res[keep], int(len(pts))

        O, place_a = np.eye(3, dtype=f32), np.zeros(3, f32)
        fetch()
        got, n_box = composed(lo, size)
        assert len(got) == n, (len(got), n)
        out["composed_equals_call"] = bool(np.array_equal(got["distance"].view(np.uint32), rec["distance"].view(np.uint32)) and
                                           np.array_equal(got["normal"].view(np.uint32), rec["normal"].view(np.uint32)))
        out["contacts"], out["candidates"], out["min_distance_cells"] = n, int(cres.candidates), round(float(cres.min_distance) / cell, 4)
        out["cell_box"] = [lo, hi]
        out["vertices_in_box"], out["vertices_in_grid"] = n_box, mesh(fetch=False)
        out["record_bytes_copied_out"] = int(rec.nbytes)
        out["composed_bytes_over_the_bus"] = {"box": n_box * (12 + 16 + 64), "grid": out["vertices_in_grid"] * (12 + 16 + 64)}
        out["count"] = median_ms(count, args.reps, args.warmup)[0]
        out["fetch"] = median_ms(fetch, args.reps, args.warmup)[0]
        out["mesh_count_box"] = median_ms(lambda: mesh(lo, size, fetch=False), args.reps, args.warmup)[0]
        out["mesh_count_grid"] = median_ms(lambda: mesh(fetch=False), args.reps, args.warmup)[0]
        out["composed"] = median_ms(lambda: composed(lo, size), args.reps, args.warmup)[0]
        out["composed_grid"] = median_ms(lambda: composed(None, None), args.reps, args.warmup)[0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
