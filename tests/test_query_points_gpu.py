"""GPU distance queries (vrt_query_points / _host, VHipRenderer.query_points / project_points) against the numpy restatement of the
rule (points_ref.py): bit for bit where the header pins every rounding (an identity instance), to 1e-5 against a float64 evaluation of
the same rule where it does not (placed instances), and as plumbing — streams, graph capture and replay across an edit, the render's
bookkeeping, deferred scene sets, undo — like the ray queries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import capacity_scenes as cs
import points_ref as P
import volumetricraytracer_amd as v
from volume_ref import dense_field
from volumetricraytracer_amd import _abi

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMATS = [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16]
TOL = 1e-5  # the ray queries' figure: distances relative to max(1, |distance|), normals absolute


@pytest.fixture(scope="module")
def pq():
    """A context of this module's own (the session renderer's scene and output size stay as other modules left them)."""
    with v.VHipRenderer() as r:
        yield r


def ref_scene(sc):
    """(slots, instances) of points_ref from the scene as the renderer uploads it."""
    slots = [P.Slot(dense_field(vol.density, vol.device_format), np.asarray(vol.material_id, np.uint8), vol.device_format, vol.VolumeExtends,
                    vol.density_scale, vol.step_max) for vol in sc.volumes()]
    a = sc.to_abi()
    inst = [P.Instance(a.instances[i].volume_slot, tuple(a.instances[i].position), tuple(a.instances[i].rotation), tuple(a.instances[i].scale))
            for i in range(a.n_instances)]
    return slots, inst


def use(r, sc):
    r.SetSceneToRender(sc)
    r.SyncWithScene()


def volume(res, extent, fn=None, fmt=_abi.FORMAT_F32, density=None):
    vol = v.VVoxelVolume(res, extent)
    if fn is not None:
        vol.fill(fn)
    if density is not None:
        vol.density = np.ascontiguousarray(density, f32)
        with np.errstate(invalid="ignore"):
            vol.material_id = (vol.density <= 0).astype(np.uint8) * 3
    return vol.set_device_format(fmt)


def sphere_fn(radius, centre=(0.0, 0.0, 0.0)):
    cx, cy, cz = (f32(c) for c in centre)
    return lambda X, Y, Z: np.sqrt(((X - cx) * (X - cx) + (Y - cy) * (Y - cy)) + (Z - cz) * (Z - cz)).astype(f32) - f32(radius)


# -- 1. bit for bit: one instance at the origin, unrotated, unscaled ------------------------------------------------------------------
EXTENT = 3.3


def identity_points(vol, seed):
    a = vol.axis_positions().astype(f32)
    E = f32(vol.VolumeExtends)
    grid = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    mid = ((a[:-1] + a[1:]) * f32(0.5)).astype(f32)
    centres = np.stack(np.meshgrid(mid, mid, mid, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    rand = rng.uniform(-1.5 * EXTENT, 1.5 * EXTENT, (2000, 3)).astype(f32)
    corners = np.array([[sx, sy, sz] for sx in (-E, E) for sy in (-E, E) for sz in (-E, E)], f32)
    faces, near = [], []
    for axis in range(3):
        for side in (-E, E):
            c = np.zeros(3, f32)
            c[axis] = side
            faces.append(c)
            for step_to in (f32(0.0), f32(np.inf) * np.sign(side)):  # one ulp inside, one ulp outside
                q = rng.uniform(-EXTENT, EXTENT, (12, 3)).astype(f32)
                q[:, axis] = np.nextafter(f32(side), step_to)
                q[0] = c
                q[0, axis] = np.nextafter(f32(side), step_to)
                near.append(q)
            last = rng.uniform(-EXTENT, EXTENT, (12, 3)).astype(f32)  # the last (or first) sample plane itself: f == 1 on the far side
            last[:, axis] = side
            near.append(last)
    return np.concatenate([grid, centres, rand, corners, np.array(faces, f32)] + near).astype(f32)


def random_field(N, seed):
    rng = np.random.default_rng(seed)
    d = (rng.normal(size=(N, N, N)) * 2.0).astype(f32)
    flat = d.reshape(-1)
    flat[rng.choice(flat.size, max(3, flat.size // 60), replace=False)] = np.nan
    flat[rng.choice(flat.size, max(3, flat.size // 60), replace=False)] = f32(-0.0)
    return d


@pytest.mark.parametrize("field", ["sphere", "random"])
@pytest.mark.parametrize("res", [2, 3, 4])
@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_instance_bit_for_bit(pq, fmt, res, field):
    N = (1 << res) + 1
    vol = volume(res, EXTENT, sphere_fn(0.6 * EXTENT), fmt) if field == "sphere" else volume(res, EXTENT, None, fmt, random_field(N, 100 + res))
    if field == "random":
        vol.material_id = np.random.default_rng(res).integers(0, 256, (N, N, N)).astype(np.uint8)
    sc = v.VScene(Objects=[v.VVoxelObject(Volume=vol)])
    use(pq, sc)
    pts = identity_points(vol, 7 * res + fmt)
    got = pq.query_points(pts)
    want = P.query(*ref_scene(sc), pts)
    assert P.same_bits(got, want) == []
    assert 0 < int(got["sampled"].sum()) < len(pts) and (got["moves"] == 0).all()
    if field == "random" and fmt == _abi.FORMAT_F32:  # a cell with a NaN corner contributes nothing, and there is no other instance
        nothing = got["instance"] == -1
        assert nothing.any() and np.isposinf(got["distance"][nothing]).all() and (got["instance"][~nothing] == 0).all()
    else:  # (the texel of NaN is 0)
        assert (got["instance"] == 0).all()
    # a projection of the same points, too
    got = pq.query_points(pts, iterations=5, tolerance=1e-3)
    want = P.query(*ref_scene(sc), pts, iterations=5, tolerance=1e-3)
    assert P.same_bits(got, want) == []


# -- 2. density_scale and step_max ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_density_scale_and_step_max(pq, fmt):
    res, N = 4, 17
    cell = 2.0 * EXTENT / (N - 1)
    thr = cell * np.sqrt(3.0)
    shell = lambda X, Y, Z: (np.abs(sphere_fn(0.5 * EXTENT)(X, Y, Z)) / f32(thr) - f32(0.5)).astype(f32)  # a Voxelizer-style shell field
    vol = volume(res, EXTENT, shell, fmt)
    rng = np.random.default_rng(21)
    pts = rng.uniform(-1.2 * EXTENT, 1.2 * EXTENT, (3000, 3)).astype(f32)
    records = {}
    for step_max in (float(f32(thr / 2)), 0.0, -1.0):
        vol.density_scale, vol.step_max = float(f32(thr)), step_max
        vol.dirty = True
        sc = v.VScene(Objects=[v.VVoxelObject(Volume=vol)])
        use(pq, sc)
        got = pq.query_points(pts)
        assert P.same_bits(got, P.query(*ref_scene(sc), pts)) == []
        records[step_max] = got
    clamped, free = records[float(f32(thr / 2))], records[0.0]
    s = clamped["sampled"]
    assert s.sum() > 1000
    assert clamped["distance"][s].max() == f32(thr / 2) and (clamped["distance"][s] == f32(thr / 2)).sum() > 100
    assert free["distance"][s].max() > 2.0 * thr  # not clamped
    assert np.array_equal(free["distance"], records[-1.0]["distance"])
    assert np.array_equal(clamped["normal"], free["normal"])  # the clamp does not touch the direction


# -- 3. placed instances ---------------------------------------------------------------------------------------------------------------
def placed_scene():
    a = volume(3, 3.3, sphere_fn(2.1), _abi.FORMAT_F32)
    box = lambda X, Y, Z: (np.maximum(np.maximum(np.abs(X) - f32(1.6), np.abs(Y) - f32(1.1)), np.abs(Z) - f32(2.0))).astype(f32)
    b = volume(4, 2.9, box, _abi.FORMAT_TEXEL16)
    b.material_id = np.random.default_rng(3).integers(0, 256, b.material_id.shape).astype(np.uint8)
    q1 = tuple(float(x) for x in v.quat_from_axis_angle((1.0, 2.0, 3.0), 0.7))
    q2 = tuple(float(x) for x in v.quat_from_axis_angle((-2.0, 0.5, 1.0), 2.1))
    q3 = tuple(float(x) for x in v.quat_from_axis_angle((0.3, -1.0, 0.2), 1.3))
    first = dict(Position=(0.4, -0.3, 0.2), Rotation=q1, Scale=(1.0, 0.8, 1.3), Volume=a)
    objs = [v.VVoxelObject(**first), v.VVoxelObject(Position=(1.9, 0.8, -0.6), Rotation=q2, Scale=(0.7, 1.2, 0.9), Volume=b),
            v.VVoxelObject(Position=(-1.5, 1.0, 1.1), Rotation=q3, Scale=(1.4, -0.9, 0.75), Volume=a), v.VVoxelObject(**first)]
    return v.VScene(Objects=objs)


def check_against_float64(got, slots, inst, pts, tol_distance, tol_normal=TOL, max_ambiguous=0.01):
    """instance, flags, voxel and material exactly, distance and normal to the tolerance, against the rule in float64 on the packed fp32
    matrices — except at points where float64 itself says that fp32 may decide otherwise: two candidates closer than the tolerance, a
    point that close to a box face, a nearest-sample tie.  Normals are compared where the gradient is long enough to give a direction
    (a twentieth of its instance's median length)."""
    want = P.evaluate(slots, inst, pts, dtype=np.float64, return_values=True)
    placements = [(I.slot, tuple(I.position), tuple(I.rotation), tuple(I.scale)) for I in inst]
    distinct = [k for k, pl in enumerate(placements) if pl not in placements[:k]]  # an exact duplicate computes the same bits: no doubt there
    vals = np.sort(np.where(np.isnan(want["values"]), np.inf, want["values"])[:, distinct], axis=1)
    scale = np.maximum(1.0, np.abs(vals[:, 0]))
    tie = (vals[:, 1] - vals[:, 0]) <= tol_distance * scale if vals.shape[1] > 1 else np.zeros(len(pts), bool)
    face = np.zeros(len(pts), bool)
    half = np.zeros(len(pts), bool)
    for k, I in enumerate(inst):
        S = slots[I.slot]
        W = P.pack_w2o(I.rotation, I.scale).astype(np.float64)
        q = (pts.astype(np.float64) - np.asarray(I.position, f32).astype(np.float64)) @ W.T
        face |= (np.abs(np.abs(q) - S.extent) <= 1e-4 * S.extent).any(axis=1)
        g = (q + S.extent) * (S.stored.shape[0] - 1) / (2.0 * S.extent)
        half |= (want["instance"] == k) & (np.abs(g + 0.5 - np.round(g + 0.5)) <= 1e-4).any(axis=1)
    ambiguous = tie | face | half
    print(f"{len(pts)} points: {int(tie.sum())} near ties, {int(face.sum())} on a face, {int(half.sum())} nearest-sample ties")
    assert ambiguous.mean() < max_ambiguous
    ok = ~ambiguous
    assert np.array_equal(got["instance"][ok], want["instance"][ok])
    assert np.array_equal(got["sampled"][ok], want["sampled"][ok])
    assert np.array_equal(got["voxel"][ok], want["voxel"][ok]) and np.array_equal(got["material"][ok], want["material"][ok])
    d = want["distance"][ok]
    assert np.all(np.abs(got["distance"][ok].astype(np.float64) - d) <= tol_distance * np.maximum(1.0, np.abs(d)))
    length = np.linalg.norm(want["h"], axis=1)
    firm = np.zeros(len(pts), bool)
    for k in range(len(inst)):
        won = want["sampled"] & (want["instance"] == k)
        if won.any():
            firm |= won & (length >= 0.05 * np.median(length[won]))
    print(f"{int((want['sampled'] & ~firm).sum())} of {int(want['sampled'].sum())} sampled points have too short a gradient to compare normals")
    assert (want["sampled"] & ~firm).sum() <= 0.02 * max(1, want["sampled"].sum())
    firm &= ok
    assert np.all(np.abs(got["normal"][firm].astype(np.float64) - want["normal"][firm]) <= tol_normal)
    assert np.all(got["normal"][ok & ~want["sampled"]] == 0)
    return want, ok


def test_placed_instances_against_the_rule_in_float64(pq):
    sc = placed_scene()
    use(pq, sc)
    slots, inst = ref_scene(sc)
    rng = np.random.default_rng(31)
    pts = rng.uniform(-6.0, 6.0, (4000, 3)).astype(f32)
    got = pq.query_points(pts)
    want, ok = check_against_float64(got, slots, inst, pts, TOL)
    assert set(got["instance"].tolist()) == {0, 1, 2}  # the duplicate at index 3 never wins: the lowest index on a tie
    assert 300 < int(got["sampled"].sum()) < 3500
    fp32 = P.query(slots, inst, pts)  # and the fp32 restatement agrees on who wins wherever float64 is sure
    assert np.array_equal(fp32["instance"][ok], got["instance"][ok])


# -- 4. capacity ------------------------------------------------------------------------------------------------------------------------
def test_capacity_64_instances_over_20_slots(pq):
    sc = cs.lattice64("mixed")
    use(pq, sc)
    slots, inst = ref_scene(sc)
    assert len(inst) == 64 and len(slots) == 20
    rng = np.random.default_rng(41)
    pts = rng.uniform(-170.0, 170.0, (3000, 3)).astype(f32)
    got = pq.query_points(pts)
    # world coordinates up to 2^8 carry 2^-16 of rounding into the object point, a scale of 0.3 multiplies it by 3.3, and a cell of 12.5
    # or 25 units spans one quantum of the field per unit: 2e-4 world units bounds the fp32 distance; the winner is exact outside that
    check_against_float64(got, slots, inst, pts, 2e-4, tol_normal=1e-4, max_ambiguous=0.02)
    assert len(set(got["instance"].tolist())) > 40


def test_coincident_pairs_name_the_lower_index_and_an_empty_scene_names_nothing(pq):
    sc = cs.coincident(0, "pairs32")
    use(pq, sc)
    rng = np.random.default_rng(42)
    pts = rng.uniform(-180.0, 180.0, (3000, 3)).astype(f32)
    got = pq.query_points(pts)
    assert (got["instance"] >= 0).all() and (got["instance"] < 32).all()  # pair j sits at indices j and 63 - j
    assert got["sampled"].sum() > 100
    empty = v.VScene(Objects=[])
    use(pq, empty)
    got = pq.query_points(pts[:300], iterations=3, tolerance=0.1)
    assert np.isposinf(got["distance"]).all() and (got["instance"] == -1).all() and not got["sampled"].any()
    assert (got["moves"] == 0).all() and (got["voxel"] == -1).all() and (got["normal"] == 0).all() and np.array_equal(got["position"], pts[:300])


# -- 5. projection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 16])
def test_a_projection_is_k_plus_one_chained_plain_queries(pq, K):
    sc = placed_scene()
    flat = volume(2, 1.5, None, _abi.FORMAT_F32, np.full((5, 5, 5), 0.75, f32))  # a constant field: no gradient, the normal is (0, 0, 0)
    sc.Objects.append(v.VVoxelObject(Position=(-4.0, -4.0, -4.0), Volume=flat))
    use(pq, sc)
    rng = np.random.default_rng(50 + K)
    pts = np.concatenate([rng.uniform(-6.0, 6.0, (3000, 3)), rng.uniform(-5.4, -2.6, (300, 3))]).astype(f32)
    tol = 2e-3
    landed = pq.query_points(pts, iterations=16, tolerance=tol)  # some points that lie within the tolerance to begin with
    on = landed["sampled"] & (np.abs(landed["distance"]) <= f32(tol))
    pts = np.concatenate([pts, landed["position"][on][:200]]).astype(f32)
    got = pq.query_points(pts, iterations=K, tolerance=tol)
    q = pts.copy()
    moves = np.zeros(len(pts), np.uint32)
    stops = {"bound": 0, "flat": 0, "near": 0}
    for _ in range(K):
        one = pq.query_points(q)
        go = P.goes_on(one, tol)
        stops["bound"] += int((~one["sampled"]).sum())
        stops["flat"] += int((one["sampled"] & (one["normal"] == 0).all(axis=1)).sum())
        stops["near"] += int((one["sampled"] & (np.abs(one["distance"]) <= f32(tol))).sum())
        q[go] = P.move(q[go], one["normal"][go], one["distance"][go])
        moves[go] += 1
    want = pq.query_points(q)
    want["moves"] = moves
    assert P.same_bits(got, want) == []
    assert all(n > 0 for n in stops.values()), stops  # every early stop occurs
    assert got["moves"].min() == 0 and (got["moves"].max() == K if K < 16 else 1 < got["moves"].max() <= K)


def test_projected_points_lie_on_the_surface_after_redistance(pq):
    res, extent = 5, 8.0
    cell = 2.0 * extent / 32
    warped = lambda X, Y, Z: (sphere_fn(5.2)(X, Y, Z) * (f32(1.5) + f32(0.08) * X)).astype(f32)  # the sphere's zero level, but no distance
    vol = volume(res, extent, warped, _abi.FORMAT_F32)
    sc = v.VScene(Objects=[v.VVoxelObject(Volume=vol)])
    p = v.default_params(64, 64, cell, v.march_budget(res, 255))
    pq.SetSceneToRender(sc)
    pq.ResizeRenderOutput(64, 64)
    pq.params_override = p
    pq.SyncWithScene()
    pq.redistance(0, vol, band=6)
    rng = np.random.default_rng(55)
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (d * rng.uniform(5.2 - 2.0 * cell, 5.2 + 2.0 * cell, (2000, 1))).astype(f32)
    tol = 1e-3 * cell
    got = pq.project_points(pts, iterations=8, tolerance=tol)
    assert got["sampled"].all() and np.all(np.abs(got["distance"]) <= f32(tol))
    rho = np.linalg.norm(got["position"].astype(np.float64), axis=1)
    # three sags add up — the warped field's zero level, redistance's, the query's: each a few hundredths of a cell — to well under half one
    assert np.all(np.abs(rho - 5.2) <= 0.5 * cell)
    back = 2.0 * cell
    origin = (got["position"] + got["normal"] * f32(back)).astype(f32)
    hits = pq.trace_rays(origin, -got["normal"], params=p)
    assert hits["hit"].all()
    assert np.all(np.abs(hits["t"] - back) <= cell)
    pq.params_override = None


# -- 6. plumbing ------------------------------------------------------------------------------------------------------------------------
def as_dict(t):
    return v.point_results_to_dict(np.ascontiguousarray(t.cpu().numpy()).view(v.POINT_RESULT_DTYPE).reshape(-1))


def to_device(pts):
    import torch

    return torch.from_numpy(v.make_points(pts).view(np.float32).reshape(-1, 4).copy()).to("cuda:0")


def carving_scene():
    vol = volume(5, 8.0, sphere_fn(5.2), _abi.FORMAT_F32)
    return v.VScene(Objects=[v.VVoxelObject(Position=(0.5, 0.0, -0.25), Volume=vol)]), vol


def test_device_buffers_streams_and_graph_replay_across_a_dab(pq):
    import torch

    sc, vol = carving_scene()
    use(pq, sc)
    rng = np.random.default_rng(61)
    pts = rng.uniform(-9.0, 9.0, (3000, 3)).astype(f32)
    n = len(pts)
    dev_pts = to_device(pts)
    out = torch.zeros((n, 16), dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pq.query_points_device(4, 1e-3, n, dev_pts.data_ptr(), out.data_ptr(), side.cuda_stream)
    side.synchronize()
    want = pq.query_points(pts, iterations=4, tolerance=1e-3)
    assert P.same_bits(as_dict(out), want) == []
    assert P.same_bits(want, P.query(*ref_scene(sc), pts, iterations=4, tolerance=1e-3)) == []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pq.query_points_device(0, 0.0, n, dev_pts.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    before = as_dict(out)
    assert P.same_bits(before, pq.query_points(pts)) == []
    res = pq.apply_brushes(0, vol, [v.sphere_brush(_abi.BRUSH_SUBTRACT, (26.0, 16.0, 16.0), 6.0)])
    assert res["written"] > 0
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    after = as_dict(out)
    assert not np.array_equal(after["distance"], before["distance"])  # the replay sees the dab
    assert P.same_bits(after, pq.query_points(pts)) == []
    assert P.same_bits(after, P.query(*ref_scene(sc), pts)) == []  # apply_brushes mirrored the written box into vol


def test_queries_leave_the_render_state_alone(pq):
    import torch

    sc = cs.lattice64("f32")
    p = cs.params(sc, w=192, h=108)
    pq.SetSceneToRender(sc)
    pq.ResizeRenderOutput(p.width, p.height)
    pq.params_override = p
    pq.SetRendererMode(p.mode)
    before = pq.Render()
    state = (pq.last_timing(), pq.timing_history(8), pq.launch_history(8), pq.last_kernel_form(), pq.wave_records(0).copy())
    pts = np.random.default_rng(62).uniform(-170.0, 170.0, (2000, 3)).astype(f32)
    dev_pts = to_device(pts)
    out = torch.zeros((len(pts), 16), dtype=torch.int32, device="cuda:0")
    for k in range(5):
        pq.query_points(pts, iterations=k, tolerance=0.01)
        pq.query_points_device(k, 0.01, len(pts), dev_pts.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    after = (pq.last_timing(), pq.timing_history(8), pq.launch_history(8), pq.last_kernel_form(), pq.wave_records(0))
    for a, b in zip(state[:4], after[:4]):
        assert a == b
    assert np.array_equal(state[4], after[4])
    assert np.array_equal(pq.Render(), before)
    pq.params_override = None


def test_queries_see_the_scene_set_while_frames_are_in_flight(pq):
    sc, vol = carving_scene()
    p = v.default_params(160, 90, vol.GetCellSize(), v.march_budget(5, 255))
    pq.SetSceneToRender(sc)
    pq.ResizeRenderOutput(p.width, p.height)
    pq.params_override = p
    pq.SyncWithScene()
    pts = np.random.default_rng(63).uniform(-12.0, 12.0, (1500, 3)).astype(f32)
    pq.render_begin(0, p)
    pq.render_begin(1, p)
    sc.Objects[0].Position = (3.5, -2.0, 1.0)
    pq.SyncWithScene()  # deferred: frames are in flight
    got = pq.query_points(pts)
    pq.render_end(0, p, copy=False)
    pq.render_end(1, p, copy=False)
    pq.params_override = None
    # a shift by fp32 numbers: the object point is p - position, then the identity matrix, so the restatement is exact again
    assert P.same_bits(got, P.query(*ref_scene(sc), pts)) == []


def test_empty_batches_and_points_that_are_not_finite(pq):
    sc, vol = carving_scene()
    use(pq, sc)
    got = pq.query_points(np.zeros((0, 3)))
    assert all(len(a) == 0 for a in got.values())
    lib, ctx = pq._lib, pq._ctx
    assert lib.vrt_query_points(ctx, 0, 0.0, 0, None, None, None) == 0
    assert lib.vrt_query_points_host(ctx, 16, 1.0, 0, None, None) == 0
    assert lib.vrt_query_points(ctx, 0, 0.0, 1, None, None, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_query_points(ctx, 17, 0.0, 0, None, None, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_query_points_host(ctx, 0, -1.0, 0, None, None) == _abi.VRT_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    pts = np.array([[nan, 0, 0], [0, inf, 0], [0, 0, -inf], [nan, nan, nan], [1.0, 2.0, 3.0], [3e38, 0, 0]], f32)
    for k in (0, 4):
        got = pq.query_points(pts, iterations=k, tolerance=1e-3)
        bad = [0, 1, 2, 3]
        assert np.isposinf(got["distance"][bad]).all() and (got["instance"][bad] == -1).all() and not got["sampled"][bad].any()
        assert (got["moves"][bad] == 0).all() and np.array_equal(got["position"][bad].view(np.uint32), pts[bad].view(np.uint32))
        assert got["instance"][4] == 0 and got["sampled"][4] and got["instance"][5] == 0 and not got["sampled"][5]
        assert P.same_bits(got, P.query(*ref_scene(sc), pts, iterations=k, tolerance=1e-3)) == []


def test_a_batch_of_1m_points(pq):
    import torch

    sc, vol = carving_scene()
    use(pq, sc)
    n = 1 << 20
    pts = np.random.default_rng(64).uniform(-10.0, 10.0, (n, 3)).astype(f32)
    got = pq.query_points(pts, iterations=2, tolerance=1e-3)
    dev_pts = to_device(pts)
    out = torch.zeros((n, 16), dtype=torch.int32, device="cuda:0")
    pq.query_points_device(2, 1e-3, n, dev_pts.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert P.same_bits(as_dict(out), got) == []
    sub = np.arange(0, n, 251)
    want = P.query(*ref_scene(sc), pts[sub], iterations=2, tolerance=1e-3)
    assert P.same_bits({k: a[sub] for k, a in got.items()}, want) == []


# -- 7. edit, undo and query -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_dab_moves_the_records_and_its_undo_restores_them_bit_for_bit(pq, fmt):
    sc, vol = carving_scene()
    vol.set_device_format(fmt)
    use(pq, sc)
    pq.enable_history(0, 8, 1 << 24)
    pts = np.random.default_rng(71).uniform(-9.0, 9.0, (3000, 3)).astype(f32)
    first = [pq.query_points(pts, iterations=k, tolerance=1e-3) for k in (0, 2)]
    res = pq.apply_brushes(0, None, [v.sphere_brush(_abi.BRUSH_SUBTRACT, (26.0, 16.0, 16.0), 6.0)])
    assert res["written"] > 0
    carved = [pq.query_points(pts, iterations=k, tolerance=1e-3) for k in (0, 2)]
    assert P.same_bits(carved[0], first[0]) != [] and P.same_bits(carved[1], first[1]) != []
    near = np.linalg.norm(pts - np.array([0.5 + 5.0, 0.0, -0.25], f32), axis=1) < 1.5  # the dab's centre lies 5 units out on the x axis
    assert near.sum() >= 3  # carving only raises the field
    assert np.all(carved[0]["distance"][near] >= first[0]["distance"][near]) and np.any(carved[0]["distance"][near] > first[0]["distance"][near])
    pq.undo(0)
    for k, want in zip((0, 2), first):
        assert P.same_bits(pq.query_points(pts, iterations=k, tolerance=1e-3), want) == []
    pq.enable_history(0, 0, 0)


# -- 8. the C++ adaptor's demo ---------------------------------------------------------------------------------------------------------
PROBE = re.compile(r"^frame (\d+) probe \(0, 0, 0\): instance (-?\d+) distance (\S+) normal \((\S+), (\S+), (\S+)\) voxel \((-?\d+), (-?\d+), (-?\d+)\) "
                   r"material (\d+) sampled ([01])$", re.M)


def test_demo_prints_one_probe_record_per_frame(tmp_path):
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    res = subprocess.run([exe, "--frames", "3", "--size", "320x180", "--probe", "0", "0", "0", "--out", str(tmp_path / "p.ppm")],
                         capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stderr
    recs = PROBE.findall(res.stdout)
    assert [int(r[0]) for r in recs] == [0, 1, 2], res.stdout
    for r in recs:
        assert int(r[1]) >= 0 and float(r[2]) > 0.0  # the origin lies outside both spheres' boxes: a box bound
        assert r[10] == "0" and [int(x) for x in r[6:9]] == [-1, -1, -1]
