"""GPU box: what a sweep query costs — 4 M seeded sweeps through the 257^3 bench shell (config 3's volume) and through a redistanced
copy of it with step_max raised to the band, at radius 0, half a cell and 2 cells (vrt_query_sweeps on device buffers; on the shell
the field is clamped to step_max, 0.87 cells, so a sphere of 2 cells is in contact wherever its centre is in the box: that leg measures
the trip to the box), against two yardsticks in the same process: vrt_trace_rays closest hit on the same origins and directions, and
the way a sweep had to be done before the call existed, chained vrt_query_points launches with a torch update between them up to the
same step cap.  Device events around the launches, a warm-up ahead, the legs take turns; prints every round and the medians, then the
step histogram and the wave efficiency — the sum of the lanes' steps over 64 x the wave's largest, which is what the lanes' different
step counts cost and what a compaction could win.  profiles/sweeps.txt keeps the output, beside the kernel's figures from the build's
ISA listing and bench.py next to the parent, which other tools make (named there)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes

N, MAX_STEPS = 1 << 22, 512
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sc = scenes.bench_config3()
vol = sc.volumes()[0]
obj = sc.Objects[0]
cell = float(vol.GetCellSize()) * float(min(abs(s) for s in obj.Scale))
p = v.default_params(1920, 1080, scenes.min_cell(sc), v.march_budget(vol.Resolution, 255), shadow=True, mode=_abi.MODE_INTERP_NOTEX)
r = v.VHipRenderer()
assert r.Start()
r.SetSceneToRender(sc)
r.ResizeRenderOutput(p.width, p.height)
r.SyncWithScene()

rng = np.random.default_rng(0)
half = vol.VolumeExtends * float(max(abs(s) for s in obj.Scale))
centre = np.asarray(obj.Position, np.float64)
away = rng.normal(size=(N, 3))
away /= np.linalg.norm(away, axis=1, keepdims=True)
origins = (centre + away * rng.uniform(1.8 * half, 2.4 * half, (N, 1))).astype(np.float32)
aims = centre + rng.uniform(-0.8 * half, 0.8 * half, (N, 3))
dirs = (aims - origins).astype(np.float32)
t_max = np.float32(6.0 * half)
tol, step_min = 1e-2 * cell, 1e-1 * cell
stream = torch.cuda.current_stream().cuda_stream


def device(a, words):
    return torch.from_numpy(a.view(np.float32).reshape(-1, words).copy()).to("cuda:0")


RADII = (0, 0.5, 2)  # cells
d_sweeps = {k: device(v.make_sweeps(origins, dirs, k * cell, t_max), 8) for k in RADII}
d_hits = torch.zeros((N, 16), dtype=torch.int32, device="cuda:0")
d_rays = device(v.make_rays(origins, dirs, t_max), 8)
d_rayhits = torch.zeros((N, 12), dtype=torch.int32, device="cuda:0")
d_o, d_d = torch.from_numpy(origins).to("cuda:0"), torch.from_numpy(dirs).to("cuda:0")
d_u = d_d / torch.linalg.norm(d_d, dim=1, keepdim=True)
d_pts = torch.zeros((N, 4), dtype=torch.float32, device="cuda:0")
d_res = torch.zeros((N, 16), dtype=torch.int32, device="cuda:0")


def chained(radius):
    """A sweep as its links: a point query per step, the update between them in torch, until no record goes on or the cap."""
    t = torch.zeros(N, dtype=torch.float32, device="cuda:0")
    active = torch.ones(N, dtype=torch.bool, device="cuda:0")
    for _ in range(MAX_STEPS):
        d_pts[:, :3] = d_o + d_u * t[:, None]
        r.query_points_device(0, 0.0, N, d_pts.data_ptr(), d_res.data_ptr(), stream)
        dist = d_res[:, 0].view(torch.float32)
        sampled = (d_res[:, 9] & 1) != 0
        c = torch.where(sampled, dist - radius, dist)
        active &= (d_res[:, 4] >= 0) & ~(sampled & (c <= tol))
        t = torch.where(active, t + torch.clamp(c, min=step_min), t)
        active &= t <= t_max
        if not bool(active.any()):  # (one read-back per link: a caller has to know when to stop)
            break
    return t


def sweep_leg(k):
    return lambda: r.sweep_spheres_device(MAX_STEPS, tol, step_min, N, d_sweeps[k].data_ptr(), d_hits.data_ptr(), stream)


legs = {
    "sweeps, radius 0": (sweep_leg(0), 3),
    "sweeps, radius 0.5 cells": (sweep_leg(0.5), 3),
    "sweeps, radius 2 cells": (sweep_leg(2), 3),
    "closest-hit rays": (lambda: r.trace_rays_device(p, _abi.QUERY_CLOSEST, N, d_rays.data_ptr(), d_rayhits.data_ptr(), stream), 5),
    "chained point queries, radius 0": (lambda: chained(0.0), 1),
    "chained point queries, radius 0.5 cells": (lambda: chained(0.5 * cell), 1),
    "chained point queries, radius 2 cells": (lambda: chained(2.0 * cell), 1),
}


def timed(fn, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n  # ms per batch


def report(title):
    print(f"== {title}: {N} sweeps, step cap {MAX_STEPS}, tolerance {tol:.4g}, step_min {step_min:.4g} (cell {cell:.4g})")
    for fn, _ in legs.values():  # clocks ramp, code objects load: untimed
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for rnd in range(rounds):
        for name, (fn, repeat) in legs.items():
            ms[name].append(timed(fn, repeat))
            print(f"round {rnd + 1} {name:38s}: {ms[name][-1]:9.4f} ms per batch -> {N / ms[name][-1] * 1e-3:9.1f} M/s")
    for name, a in ms.items():
        a = np.array(a)
        print(f"{name:38s}: median {np.median(a):9.4f} ms, min {a.min():9.4f}, max {a.max():9.4f} over {rounds} rounds -> {N / np.median(a) * 1e-3:9.1f} M/s")
    for k in RADII:
        sweep_leg(k)()
        torch.cuda.synchronize()
        res = v.sweep_hits_to_dict(np.ascontiguousarray(d_hits.cpu().numpy()).view(v.SWEEP_HIT_DTYPE).reshape(-1))
        steps = res["steps"].astype(np.int64)
        waves = steps.reshape(-1, 64)
        efficiency = waves.sum() / (64.0 * waves.max(axis=1).sum())
        edges = [0, 1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 513]
        hist = np.histogram(steps, bins=edges)[0]
        print(f"radius {k} cells: hit {res['hit'].mean():.3f}, exhausted {res['exhausted'].mean():.4f}, miss {(res['flags'] == 0).mean():.3f}; "
              f"steps mean {steps.mean():.2f}, median {np.median(steps):.0f}, largest {steps.max()}")
        print(f"   steps histogram {dict(zip([f'{a}..{b - 1}' for a, b in zip(edges[:-1], edges[1:])], hist.tolist()))}")
        print(f"   wave efficiency (sum of lane steps / 64 x the wave's largest): {efficiency:.3f}; mean of a wave's largest {waves.max(axis=1).mean():.2f}")


report("the bench shell (density_scale / step_max: a safe lower bound)")
got = r.redistance(0, None, band=15, from_=_abi.REDISTANCE_FROM_OUTSIDE)
# the field is now the distance within 15 cells of the surface and 15 cells beyond: that is how far a sample may be trusted
_abi.check(r._lib.vrt_volume_set_metric(r._ctx, 0, float(vol.density_scale), 15.0 * float(vol.GetCellSize())), "vrt_volume_set_metric")
print(f"redistanced: {got['written']} samples written; step_max {float(vol.step_max):.4g} -> {15.0 * float(vol.GetCellSize()):.4g}")
report("the redistanced copy (a true distance within 15 cells)")
r.Stop()
