"""GPU probe (not part of the suite): throughput of the ray queries (vrt_trace_rays, closest hit and occlusion) on three workloads,
next to the render kernel of the same frame:
  - config 3 (bench.py's 256^3 voxelized torus, 1920x1080): the frame's camera rays (vrt_camera_rays) as a ray buffer;
  - the same rays shuffled (incoherent: neighbouring lanes march unrelated rays);
  - config 5 (8 instanced 128^3 volumes, the BVH walk): the frame's camera rays.
Device-event time of --reps launches after --warmup, one query launch per timed interval; reports the median and the min..max spread
in Grays/s (rays per second).  The render line is vrt_render_rows of the whole frame (camera rays + directional shadow rays +
shading), counted in camera rays per second.  Writes the table to profiles/ray_query.txt (--out) and prints one JSON line.

    python tools/ray_query_probe.py [--reps 20] [--warmup 5] [--out profiles/ray_query.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import volumetricraytracer_amd as v  # noqa: E402
from volumetricraytracer_amd import _abi  # noqa: E402
from volumetricraytracer_amd import workloads  # noqa: E402

W, H = 1920, 1080


def timed(torch, fn, reps, warmup):
    """Median and spread (ms) of device-event-timed calls of fn on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def rate(n, t):
    med, lo, hi = t
    return {"ms": round(med, 4), "grays_s": round(n / med * 1e-6, 3), "spread_grays_s": [round(n / hi * 1e-6, 3), round(n / lo * 1e-6, 3)]}


def workload(torch, r, sc, reps, warmup, shuffle_too=False):
    max_steps = v.march_budget(max(vol.Resolution for vol in sc.volumes()), 255)
    p = v.default_params(W, H, workloads.min_cell(sc), max_steps, shadow=True)
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(W, H)
    r.params_override = p
    r.SetRendererMode(p.mode)
    r.SyncWithScene()
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    out = {"render_rows": rate(W * H, timed(torch, lambda: r.render_rows(p, 0, H, frame.data_ptr(), stream), reps, warmup))}
    px = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)  # row-major pixel order, as the frame
    host = r.camera_rays(px, W, H)
    sets = [("camera_rays", host)]
    if shuffle_too:
        sets.append(("camera_rays_shuffled", host[np.random.default_rng(0).permutation(len(host))]))
    hits = torch.zeros((len(host), 12), dtype=torch.int32, device="cuda:0")
    for name, rays_np in sets:
        rays = torch.from_numpy(rays_np.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
        for qname, q in (("closest", _abi.QUERY_CLOSEST), ("any", _abi.QUERY_ANY)):
            t = timed(torch, lambda: r.trace_rays_device(p, q, len(rays_np), rays.data_ptr(), hits.data_ptr(), stream), reps, warmup)
            out[f"{name}_{qname}"] = rate(len(rays_np), t)
        got = np.ascontiguousarray(hits.cpu().numpy()).view(v.HIT_DTYPE).reshape(-1)
        out[f"{name}_hit_fraction_any"] = round(float(np.mean(got["instance"] >= 0)), 4)
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query.txt"))
    args = ap.parse_args()
    res = {"frame": f"{W}x{H}", "reps": args.reps, "unit": "Grays/s = rays per second / 1e9 (render_rows: camera rays), median of device-event "
                                                          "times, spread = [slowest, fastest] launch"}
    with v.VHipRenderer() as r:
        res["config3_256"] = workload(torch, r, workloads.bench_config3(), args.reps, args.warmup, shuffle_too=True)
        res["config5_bvh"] = workload(torch, r, workloads.config5_instances(7, 256), args.reps, args.warmup)
    lines = ["# tools/ray_query_probe.py: vrt_trace_rays throughput on one MI355X, " + res["unit"] + f"; {args.reps} timed launches after "
             f"{args.warmup} warm-up each", f"# frame {res['frame']}; closest = VRT_QUERY_CLOSEST, any = VRT_QUERY_ANY (t_max 10000)"]
    for wl in ("config3_256", "config5_bvh"):
        for k, x in res[wl].items():
            if isinstance(x, dict):
                lines.append(f"{wl:12s} {k:30s} {x['grays_s']:8.3f} Grays/s  ({x['spread_grays_s'][0]:.3f} .. {x['spread_grays_s'][1]:.3f})  "
                             f"{x['ms']:.4f} ms")
            else:
                lines.append(f"{wl:12s} {k:30s} {x}")
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
