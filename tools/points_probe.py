"""GPU box: what a distance query costs — 4 M random points in and around the 256^3 bench shell (config 3's volume) as a plain query and
as an 8-iteration projection (vrt_query_points on device buffers), and, as the yardstick, vrt_trace_rays of 4 M rays through the same
volume in the same process.  Device events around batches of launches, a warm-up ahead, interleaved rounds; prints every round and the
spread."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes

N_POINTS, REPEAT = 1 << 22, 5
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sc = scenes.bench_config3()
vol = sc.volumes()[0]
obj = sc.Objects[0]
p = v.default_params(1920, 1080, scenes.min_cell(sc), v.march_budget(vol.Resolution, 255), shadow=True, mode=_abi.MODE_INTERP_NOTEX)
r = v.VHipRenderer()
assert r.Start()
r.SetSceneToRender(sc)
r.ResizeRenderOutput(p.width, p.height)
r.SyncWithScene()

rng = np.random.default_rng(0)
reach = 1.25 * vol.VolumeExtends * float(max(abs(s) for s in obj.Scale))  # a quarter of the points fall outside the box
pts = (np.asarray(obj.Position, np.float32) + rng.uniform(-reach, reach, (N_POINTS, 3))).astype(np.float32)
dirs = rng.normal(size=(N_POINTS, 3)).astype(np.float32)
d_pts = torch.from_numpy(v.make_points(pts).view(np.float32).reshape(-1, 4).copy()).to("cuda:0")
d_res = torch.zeros((N_POINTS, 16), dtype=torch.int32, device="cuda:0")
d_rays = torch.from_numpy(v.make_rays(pts, dirs).view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
d_hits = torch.zeros((N_POINTS, 12), dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream().cuda_stream
tol = 1e-3 * float(vol.GetCellSize())

legs = {
    "plain query": lambda: r.query_points_device(0, 0.0, N_POINTS, d_pts.data_ptr(), d_res.data_ptr(), stream),
    "projection, 8 iterations": lambda: r.query_points_device(8, tol, N_POINTS, d_pts.data_ptr(), d_res.data_ptr(), stream),
    "closest-hit rays": lambda: r.trace_rays_device(p, _abi.QUERY_CLOSEST, N_POINTS, d_rays.data_ptr(), d_hits.data_ptr(), stream),
}


def timed(fn, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n  # ms per launch


for fn in legs.values():  # clocks ramp, code objects load: untimed
    timed(fn, 3)
rates = {name: [] for name in legs}
for rnd in range(rounds):
    for name, fn in legs.items():
        ms = timed(fn, REPEAT)
        rates[name].append(N_POINTS / ms * 1e-6)  # G per second
        print(f"round {rnd + 1} {name:26s}: {ms:.4f} ms per {N_POINTS} -> {rates[name][-1]:.3f} G/s")
res = v.point_results_to_dict(np.ascontiguousarray(d_res.cpu().numpy()).view(v.POINT_RESULT_DTYPE).reshape(-1))
print(f"projection: sampled {res['sampled'].mean():.3f} of the points, moves {np.bincount(res['moves'], minlength=9).tolist()}, "
      f"within tolerance {(np.abs(res['distance'][res['sampled']]) <= tol).mean():.3f} of the sampled")
for name, g in rates.items():
    g = np.array(g)
    print(f"{name:26s}: median {np.median(g):.3f} G/s, min {g.min():.3f}, max {g.max():.3f} over {rounds} rounds of {REPEAT} launches")
r.Stop()
