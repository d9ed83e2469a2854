"""GPU ray queries (vrt_trace_rays / _host, VHipRenderer.trace_rays / pick) against the CPU oracle: every closest hit is the
oracle's vrto_trace of the same ray (hit flag, instance and steps exactly, t and normal to 1e-5; the march is the render's, bit for
bit in practice), occlusion agrees with the oracle's hit flags, the voxel and material of a hit are recomputed here from the
oracle's t, and queries are capturable, see region edits and leave the render's state alone."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from oracle.binding import OracleScene

pytestmark = pytest.mark.gpu
TTOL = 1e-5  # t: relative to max(1, t); normal: absolute


@pytest.fixture(scope="module")
def rq(oracle_lib):
    """A context of this module's own (the session renderer's output size and params stay as other modules left them)."""
    with v.VHipRenderer() as r:
        yield r


def use(r, sc, p):
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)
    r.SyncWithScene()


def params(sc, mode=_abi.MODE_INTERP_NOTEX, path=_abi.PATH_AUTO, flags=0, w=96, h=54):
    p = v.default_params(w, h, scenes.min_cell(sc), v.march_budget(max(vol.Resolution for vol in sc.volumes()), 255), shadow=True,
                         mode=mode, path=path)
    p.flags = flags
    return p


def instance_frames(sc):
    """Per instance (in vrt_scene order): position, rotation quaternion, scale, volume."""
    return [(np.asarray(o.Position, np.float64), o.Rotation, np.asarray(o.Scale, np.float64), o.Volume) for o in sc.Objects
            if isinstance(o, v.VVoxelObject) and o.Volume is not None]


def to_world(inst, p_obj):
    pos, rot, scale, _ = inst
    return pos + scale * v.quat_rotate(rot, p_obj).astype(np.float64)


def to_object(inst, p_world):
    """w2o = R^T S^-1 (csrc/vrt_api.hip pack_instance)."""
    pos, rot, scale, _ = inst
    return v.quat_rotate(v.quat_inverse(rot), (np.asarray(p_world, np.float64) - pos) / scale).astype(np.float64)


def query_rays(r, sc, p, n_random=1500, seed=0):
    """A frame's camera rays (every pixel of p's frame) and seeded random rays from outside and inside the volumes, a quarter of
    those from solid cells (density <= 0)."""
    W, H = p.width, p.height
    cam = r.camera_rays([(x, y) for y in range(H) for x in range(W)], W, H)
    rng = np.random.default_rng(seed)
    insts = instance_frames(sc)
    solids = {}
    o, d = [], []
    for k in range(n_random):
        inst = insts[k % len(insts)]
        vol = inst[3]
        E = vol.VolumeExtends
        if k % 4 == 0:  # a solid cell's sample point
            if id(vol) not in solids:
                solids[id(vol)] = np.argwhere(vol.density <= 0.0)
            solid = solids[id(vol)]
            x, z, y = solid[rng.integers(len(solid))] if len(solid) else (vol.N // 2,) * 3
            p_obj = np.array([x, y, z], np.float64) * vol.GetCellSize() - E
        else:
            p_obj = rng.uniform(-1.6 * E, 1.6 * E, 3)
        o.append(to_world(inst, p_obj))
        d.append(rng.normal(size=3))
    o = np.concatenate([cam["origin"], np.asarray(o, np.float32)])
    d = np.concatenate([cam["direction"], np.asarray(d, np.float32)])
    return o.astype(np.float32), d.astype(np.float32)


def compare(r, sc, p, o, d, t_max=10000.0, n_single=24, seed=1, got=None):
    """GPU closest hits of (o, d) against oracle trace_batch (hit, t, normal) and single-ray trace (instance, steps) on a subset."""
    osc = OracleScene(sc)
    got = got if got is not None else r.trace_rays(o, d, t_max, params=p)
    hit, t, nrm = osc.trace_batch(p, o, d, t_max, threads=16)
    assert np.array_equal(got["hit"], hit), f"{int(np.sum(got['hit'] != hit))} of {len(hit)} hit flags differ"
    assert np.all(np.abs(got["t"][hit] - t[hit]) <= TTOL * np.maximum(1.0, np.abs(t[hit])))
    assert np.all(np.abs(got["normal"][hit] - nrm[hit]) <= TTOL)
    assert np.all(got["t"][~hit] == -1.0) and np.all(got["normal"][~hit] == 0.0)
    assert np.all(got["instance"][~hit] == -1) and np.all(got["voxel"][~hit] == -1) and np.all(got["material"][~hit] == 0)
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.choice(np.flatnonzero(hit), min(n_single // 2, int(hit.sum())), replace=False),
                          rng.choice(len(o), n_single // 2, replace=False)])
    single = len(instance_frames(sc)) == 1
    for k in idx:
        h, tk, _, inst, steps = osc.trace(p, o[k], d[k], t_max)
        assert got["instance"][k] == (inst if h else -1), k
        if single:
            assert int(got["steps"][k]) == steps, (k, int(got["steps"][k]), steps)
        elif p.mode < _abi.MODE_CUBE:
            # the BVH walk skips instances whose box lies beyond the closest hit so far; the oracle marches every instance the ray
            # meets, each with the same interval: a subset of its positions (test_parity_gpu's config 5 parity makes the same exception)
            assert int(got["steps"][k]) <= steps, (k, int(got["steps"][k]), steps)
    return got, hit, t


def hit_pixel(r, p):
    """The pixel nearest the frame's centre whose camera ray hits something (the torus' centre pixel looks through its hole)."""
    W, H = p.width, p.height
    px = np.array([(x, y) for y in range(H) for x in range(W)], np.int32)
    cam = r.camera_rays(px, W, H)
    hit = r.trace_rays(cam["origin"], cam["direction"], params=p)["hit"]
    k = np.flatnonzero(hit)[np.argmin(((px[hit] - [W // 2, H // 2]) ** 2).sum(1))]
    return int(px[k][0]), int(px[k][1])


# -- closest-hit parity ---------------------------------------------------------------------------------------------------------
PATHS = (_abi.PATH_AUTO, _abi.PATH_DENSE, _abi.PATH_BRICK, _abi.PATH_BRICK_LDS, _abi.PATH_CELLS)
FLAGS = (0, _abi.FLAG_NO_HIT_POLISH, _abi.FLAG_REFERENCE_BOUNDARY_TEXELS)


def shell_scene(res, fmt):
    """Config 3's voxelized torus (a shell field with both empty-space table levels) in device format fmt."""
    return scenes.config3_voxelized(res, 16, device_format=fmt)


@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
@pytest.mark.parametrize("path", PATHS)
def test_closest_hits_every_path_interp(rq, fmt, path):
    sc = shell_scene(6, fmt)
    for k, flags in enumerate(FLAGS):
        p = params(sc, path=path, flags=flags)
        use(rq, sc, p)
        o, d = query_rays(rq, sc, p, seed=k)
        compare(rq, sc, p, o, d, seed=k)


@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
def test_closest_hits_cube_modes(rq, fmt):
    sc = shell_scene(6, fmt)
    for k, (mode, flags) in enumerate([(_abi.MODE_CUBE_NOTEX, 0), (_abi.MODE_CUBE, _abi.FLAG_NO_HIT_POLISH),
                                       (_abi.MODE_CUBE_NOTEX_UNLIT, _abi.FLAG_REFERENCE_BOUNDARY_TEXELS)]):
        p = params(sc, mode=mode, flags=flags)
        use(rq, sc, p)
        o, d = query_rays(rq, sc, p, seed=10 + k)
        compare(rq, sc, p, o, d, seed=k)


@pytest.mark.parametrize("which", ["config2", "config3_analytic", "config3_texel16_cone0"])
def test_closest_hits_configs(rq, which):
    if which == "config2":
        sc = scenes.config2_sphere(6, 16)
        p = params(sc)
    elif which == "config3_analytic":
        sc = scenes.config3_torus(6, 16)
        p = params(sc, flags=_abi.FLAG_REFERENCE_BOUNDARY_TEXELS)
    else:
        sc = shell_scene(6, _abi.FORMAT_TEXEL16)
        p = params(sc, path=_abi.PATH_CELLS)
        p.cone_eps = 0.0  # a constant threshold
    use(rq, sc, p)
    o, d = query_rays(rq, sc, p)
    compare(rq, sc, p, o, d)


def test_closest_hits_on_the_256_cubed_bench_shell(rq):
    sc = scenes.bench_config3()
    for k, (mode, path) in enumerate([(_abi.MODE_INTERP_NOTEX, _abi.PATH_AUTO), (_abi.MODE_CUBE_NOTEX, _abi.PATH_AUTO)]):
        p = params(sc, mode=mode, path=path, w=64, h=36)
        use(rq, sc, p)
        o, d = query_rays(rq, sc, p, n_random=600, seed=k)
        compare(rq, sc, p, o, d, n_single=6, seed=k)


@pytest.mark.parametrize("distinct", [False, True])
def test_closest_hits_config5(rq, distinct):
    sc = scenes.config5_instances(5, 16, distinct_volumes=distinct)
    for k, (mode, path, flags) in enumerate([(_abi.MODE_INTERP_NOTEX, _abi.PATH_AUTO, 0),
                                             (_abi.MODE_INTERP_NOTEX, _abi.PATH_DENSE, _abi.FLAG_REFERENCE_BOUNDARY_TEXELS),
                                             (_abi.MODE_CUBE_NOTEX, _abi.PATH_AUTO, _abi.FLAG_NO_HIT_POLISH)]):
        p = params(sc, mode=mode, path=path, flags=flags)
        use(rq, sc, p)
        o, d = query_rays(rq, sc, p, seed=k)
        got, hit, _ = compare(rq, sc, p, o, d, seed=k)
        assert len(set(got["instance"][hit].tolist())) >= 4  # several instances are hit


def test_per_ray_t_max(rq):
    sc = scenes.config5_instances(5, 16)
    p = params(sc)
    use(rq, sc, p)
    o, d = query_rays(rq, sc, p, seed=3)
    buckets = np.array([0.0, 40.0, 700.0, 900.0, 1100.0, 10000.0], np.float32)
    which = np.random.default_rng(4).integers(0, len(buckets), len(o))
    got = rq.trace_rays(o, d, buckets[which], params=p)
    for b, t_max in enumerate(buckets):
        sel = which == b
        sub = {k: a[sel] for k, a in got.items()}
        compare(rq, sc, p, o[sel], d[sel], float(t_max), n_single=6, seed=b, got=sub)
    assert 0 < int(got["hit"].sum()) < len(o)


def test_occlusion_agrees_with_the_oracles_hit_flags(rq):
    sc = scenes.config5_instances(5, 16, distinct_volumes=True)
    p = params(sc)
    use(rq, sc, p)
    o, d = query_rays(rq, sc, p, seed=5)
    osc = OracleScene(sc)
    for t_max in (60.0, 400.0, 10000.0):
        got = rq.trace_rays(o, d, t_max, any_hit=True, params=p)
        hit, _, _ = osc.trace_batch(p, o, d, t_max, threads=16)
        assert np.array_equal(got["hit"], hit)
        assert np.all(got["instance"][hit] == 0) and np.all(got["t"] == -1.0) and np.all(got["normal"] == 0.0)
        assert np.all(got["voxel"] == -1) and np.all(got["material"] == 0)
    # line of sight between pairs of points: blocked when the segment from a to b meets a surface
    rng = np.random.default_rng(6)
    a = rng.uniform(-350.0, 350.0, (3000, 3)).astype(np.float32)
    b = rng.uniform(-350.0, 350.0, (3000, 3)).astype(np.float32)
    seg = (b - a).astype(np.float32)
    length = np.sqrt((seg.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    got = rq.trace_rays(a, seg, length, any_hit=True, params=p)
    want = np.array([osc.trace(p, a[k], seg[k], float(length[k]))[0] for k in range(200)])
    assert np.array_equal(got["hit"][:200], want)
    for k in range(200, 3000, 700):
        blocked = rq.trace_rays(a[k:k + 1], seg[k:k + 1], length[k], any_hit=True, params=p)["hit"][0]
        assert blocked == got["hit"][k]
    assert 0 < int(got["hit"].sum()) < len(a)


@pytest.mark.parametrize("which", ["config3", "config5"])
def test_voxel_and_material_of_a_hit(rq, which):
    sc = shell_scene(6, _abi.FORMAT_F32) if which == "config3" else scenes.config5_instances(5, 16, distinct_volumes=True)
    rng = np.random.default_rng(7)
    for vol in sc.volumes():
        vol.material_id = rng.integers(0, 256, vol.material_id.shape).astype(np.uint8)
    p = params(sc)
    use(rq, sc, p)
    o, d = query_rays(rq, sc, p, seed=8)
    got, hit, t = compare(rq, sc, p, o, d, seed=8)
    insts = instance_frames(sc)
    dn = d.astype(np.float64) / np.sqrt((d.astype(np.float64) ** 2).sum(1, keepdims=True))
    checked = 0
    for k in np.flatnonzero(hit):
        inst = insts[got["instance"][k]]
        vol = inst[3]
        p_obj = to_object(inst, o[k].astype(np.float64) + dn[k] * float(t[k]))
        u = (p_obj + vol.VolumeExtends) / vol.GetCellSize()
        if np.any(np.abs(u - np.floor(u) - 0.5) < 1e-3):
            continue  # a half-cell tie
        want = np.clip(np.floor(u + 0.5), 0, vol.N - 1).astype(int)
        assert got["voxel"][k].tolist() == want.tolist(), (k, got["voxel"][k], want)
        assert got["material"][k] == vol.material_id[want[0], want[2], want[1]]
        checked += 1
    assert checked > 0.9 * hit.sum() > 0


def test_pick_edit_and_query_again(rq):
    sc = shell_scene(6, _abi.FORMAT_F32)
    vol = sc.volumes()[0]
    p = params(sc, w=160, h=90)
    use(rq, sc, p)
    cx, cy = hit_pixel(rq, p)
    h0 = rq.pick(cx, cy)
    assert h0["hit"] and h0["instance"] == 0
    o, d = OracleScene(sc).camera_rays(160, 90, [(cx, cy)])
    hit, t, nrm, inst, steps = OracleScene(sc).trace(p, o[0], d[0])
    assert hit and abs(h0["t"] - t) <= TTOL * t and int(h0["steps"]) == steps
    # carve a ball of 4 cells around the picked voxel
    c = h0["voxel"]
    rad = 4
    lo = np.maximum(c - rad, 0)
    hi = np.minimum(c + rad, vol.N - 1)
    cell = vol.GetCellSize()
    for x in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for z in range(lo[2], hi[2] + 1):
                carved = (rad - math.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)) * cell
                vol.density[x, z, y] = max(vol.density[x, z, y], carved)
    rq.update_volume_region(0, vol, tuple(int(a) for a in lo), tuple(int(a) for a in hi))
    h1 = rq.pick(cx, cy)
    assert (not h1["hit"]) or h1["t"] > h0["t"]  # deeper, or through
    hit1, t1, _, inst1, steps1 = OracleScene(sc).trace(p, o[0], d[0])
    assert h1["hit"] == hit1 and int(h1["steps"]) == steps1
    if hit1:
        assert abs(h1["t"] - t1) <= TTOL * t1
    ro, rd = query_rays(rq, sc, p, n_random=400, seed=9)
    compare(rq, sc, p, ro, rd, n_single=8)


def test_device_buffers_streams_and_graph_replay(rq):
    import torch

    sc = shell_scene(6, _abi.FORMAT_F32)
    vol = sc.volumes()[0]
    p = params(sc)
    p.flags |= _abi.FLAG_NO_CULL_RECT
    use(rq, sc, p)
    o, d = query_rays(rq, sc, p, n_random=1000, seed=11)
    n = len(o)
    host_rays = v.make_rays(o, d)
    rays = torch.from_numpy(host_rays.view(np.float32).reshape(n, 8).copy()).to("cuda:0")
    hits = torch.zeros((n, 12), dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rq.trace_rays_device(p, _abi.QUERY_CLOSEST, n, rays.data_ptr(), hits.data_ptr(), side.cuda_stream)
    side.synchronize()

    def as_dict(t):
        return v.hits_to_dict(np.ascontiguousarray(t.cpu().numpy()).view(v.HIT_DTYPE).reshape(-1))

    want = rq.trace_rays(o, d, params=p)
    got = as_dict(hits)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rq.trace_rays_device(p, _abi.QUERY_CLOSEST, n, rays.data_ptr(), hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    # a replay after rewriting the ray buffer
    rng = np.random.default_rng(12)
    d2 = rng.normal(size=(n, 3)).astype(np.float32)
    o2 = (o + rng.normal(scale=5.0, size=(n, 3))).astype(np.float32)
    rays.copy_(torch.from_numpy(v.make_rays(o2, d2).view(np.float32).reshape(n, 8).copy()))
    hits.zero_()
    g.replay()
    torch.cuda.synchronize()
    got2 = as_dict(hits)
    want2 = rq.trace_rays(o2, d2, params=p)
    for k in want2:
        assert np.array_equal(got2[k], want2[k]), k
    compare(rq, sc, p, o2, d2, n_single=6, got=got2)
    # a replay after a region edit: a slab through the torus removed
    lo, hi = (0, 20, 0), (vol.N - 1, 44, vol.N - 1)
    vol.density[:, :, 20:45] = np.maximum(vol.density[:, :, 20:45], 5.0 * vol.GetCellSize())
    rq.update_volume_region(0, vol, lo, hi)
    hits.zero_()
    g.replay()
    torch.cuda.synchronize()
    got3 = as_dict(hits)
    assert not np.array_equal(got3["hit"], got2["hit"])
    compare(rq, sc, p, o2, d2, n_single=6, got=got3)


def test_queries_leave_the_render_state_alone(rq):
    import torch

    sc = scenes.config5_instances(5, 16)
    p = params(sc, w=192, h=108)
    p.flags |= _abi.FLAG_OUTPUT_RGBA8
    use(rq, sc, p)
    before = rq.Render()
    state = (rq.last_timing(), rq.timing_history(8), rq.launch_history(8), rq.last_kernel_form(), rq.wave_records(0).copy())
    o, d = query_rays(rq, sc, p, n_random=500, seed=13)
    rays = torch.from_numpy(v.make_rays(o, d).view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
    hits = torch.zeros((len(o), 12), dtype=torch.int32, device="cuda:0")
    for k in range(5):
        rq.trace_rays(o, d, params=p, any_hit=bool(k % 2))
        rq.trace_rays_device(p, k % 2, len(o), rays.data_ptr(), hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    after = (rq.last_timing(), rq.timing_history(8), rq.launch_history(8), rq.last_kernel_form(), rq.wave_records(0))
    for a, b in zip(state[:4], after[:4]):
        assert a == b
    assert np.array_equal(state[4], after[4])
    assert np.array_equal(rq.Render(), before)


def test_queries_see_the_scene_set_while_frames_are_in_flight(rq):
    sc = shell_scene(6, _abi.FORMAT_F32)
    p = params(sc, w=160, h=90)
    use(rq, sc, p)
    o, d = query_rays(rq, sc, p, n_random=300, seed=14)
    rq.render_begin(0, p)
    rq.render_begin(1, p)
    obj = sc.Objects[0]
    obj.Position = (obj.Position[0] + 30.0, obj.Position[1] - 10.0, obj.Position[2])
    rq.SyncWithScene()  # deferred: frames are in flight
    got = rq.trace_rays(o, d, params=p)
    rq.render_end(0, p, copy=False)
    rq.render_end(1, p, copy=False)
    compare(rq, sc, p, o, d, n_single=8, got=got)


# -- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_a_context_of_the_same_device_three_times(rq):
    sc = scenes.config5_instances(5, 16)
    p = params(sc)
    use(rq, sc, p)
    o, d = query_rays(rq, sc, p, n_random=500, seed=15)
    want = rq.trace_rays(o, d, params=p)
    with v.VHipRenderer(devices=(0, 0, 0)) as r3:
        use(r3, sc, p)
        got = r3.trace_rays(o, d, params=p)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_empty_batches_and_bad_rays(rq):
    sc = shell_scene(6, _abi.FORMAT_F32)
    p = params(sc)
    use(rq, sc, p)
    got = rq.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)), params=p)
    assert all(len(a) == 0 for a in got.values())
    assert rq._lib.vrt_trace_rays(rq._ctx, C.byref(p), _abi.QUERY_CLOSEST, 0, None, None, None) == 0
    assert rq._lib.vrt_trace_rays(rq._ctx, C.byref(p), _abi.QUERY_ANY, 0, None, None, None) == 0
    assert rq._lib.vrt_trace_rays(rq._ctx, C.byref(p), 7, 0, None, None, None) == _abi.VRT_ERR_INVALID
    assert rq._lib.vrt_trace_rays(rq._ctx, C.byref(p), _abi.QUERY_CLOSEST, -1, None, None, None) == _abi.VRT_ERR_INVALID
    assert rq._lib.vrt_trace_rays(rq._ctx, C.byref(p), _abi.QUERY_CLOSEST, 1, None, None, None) == _abi.VRT_ERR_INVALID
    centre = rq.camera_rays([hit_pixel(rq, p)])  # a ray that hits the torus
    cam, fwd = centre["origin"][0], centre["direction"][0]
    nan, inf = float("nan"), float("inf")
    o = np.array([cam] * 7 + [[nan, 0, 0], [0, inf, 0], cam], np.float32)
    d = np.array([[0, 0, 0], [nan, 0, 0], [inf, 0, 0], [-1, -inf, 0], [0, 0, nan], fwd * 1e-10, fwd * 1e15, fwd, fwd, fwd], np.float32)
    t_max = np.array([1e4] * 9 + [nan], np.float32)
    for any_hit in (False, True):
        got = rq.trace_rays(o, d, t_max, any_hit=any_hit, params=p)
        bad = [0, 1, 2, 3, 4, 7, 8, 9]  # zero / non-finite directions, non-finite origins, a NaN t_max
        assert not got["hit"][bad].any() and np.all(got["steps"][bad] == 0) and np.all(got["t"][bad] == -1.0)
        assert np.all(got["instance"][bad] == -1)
        assert got["hit"][5] and got["hit"][6]  # a tiny or a huge direction is still a direction


def test_a_batch_of_4m_rays(rq):
    import torch

    sc = shell_scene(6, _abi.FORMAT_F32)
    p = params(sc)
    use(rq, sc, p)
    n = 1 << 22
    rng = np.random.default_rng(16)
    o = rng.uniform(-160.0, 160.0, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    got = rq.trace_rays(o, d, params=p)
    assert 0 < int(got["hit"].sum()) < n
    rays = torch.from_numpy(v.make_rays(o, d).view(np.float32).reshape(n, 8).copy()).to("cuda:0")
    hits = torch.zeros((n, 12), dtype=torch.int32, device="cuda:0")
    rq.trace_rays_device(p, _abi.QUERY_CLOSEST, n, rays.data_ptr(), hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dev = np.ascontiguousarray(hits.cpu().numpy()).view(v.HIT_DTYPE).reshape(-1)
    assert np.array_equal(dev["instance"], got["instance"]) and np.array_equal(dev["t"], got["t"]) and np.array_equal(dev["steps"], got["steps"])
    sub = np.arange(0, n, 997)
    compare(rq, sc, p, o[sub], d[sub], n_single=6, got={k: a[sub] for k, a in got.items()})


# -- the C++ adaptor's demo -------------------------------------------------------------------------------------------------------
PICK = re.compile(r"^frame (\d+) pick \(160, 90\): instance (-?\d+) t (\S+) normal \((\S+), (\S+), (\S+)\) voxel \((-?\d+), (-?\d+), (-?\d+)\) "
                  r"material (\d+) steps (\d+)$", re.M)


def test_demo_prints_one_pick_record_per_frame(tmp_path):
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    outs = []
    for k, extra in enumerate([[], ["--edit-brush", "4"], ["--edit-brush", "4"]]):
        res = subprocess.run([exe, "--frames", "3", "--size", "320x180", "--pick", "160", "90", "--out", str(tmp_path / f"{k}.ppm")] + extra,
                             capture_output=True, text=True, timeout=180)
        assert res.returncode == 0, res.stderr
        recs = PICK.findall(res.stdout)
        assert [int(r[0]) for r in recs] == [0, 1, 2], res.stdout
        for r in recs:
            assert int(r[1]) >= 0 and float(r[2]) > 0.0
            assert all(0 <= int(x) < 65 for x in r[6:9])  # the demo's spheres: 2^6 + 1 samples per axis
        outs.append(recs)
    assert outs[1] == outs[2]  # the brush follows the pick deterministically
    assert float(outs[1][2][2]) >= float(outs[0][2][2])  # the brush dug in where the pick looked
