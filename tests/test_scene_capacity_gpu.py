"""GPU parity at the limits include/vrt.h promises — 64 instances, 20 volumes, 5 + 5 lights — and on the scenes that corner the
wave-walked instance BVH (capacity_scenes.py; what each scene contains is asserted on the oracle alone in test_scene_capacity.py).

Yardstick: the CPU oracle's brute-force visit (every instance in index order, strict t < best, no BVH): every pixel within the
suite's 1e-4, no NaN; primary_rays, shadow_rays, bounce_rays and hits exact; ray queries by test_ray_query_gpu.py's rule (hit flag
and instance exact, t and normal to 1e-5).  Every frame is rendered as one kernel (VRT_FLAG_FULL_ONE_KERNEL) and in passes
(VRT_FLAG_FULL_THREE_PASS): the two are bit-equal with equal counters.

Step counters.  In the sphere-trace modes primary_steps <= the oracle's: a closest-hit walk marches an instance only when the ray
meets its world box within the closest hit so far, the oracle marches every instance, and a visited instance's march is the
oracle's (it covers the instance's whole interval, whatever was hit before), so the kernel's marches are a subset of the oracle's.
The bound does NOT hold for shadow_steps and is not asserted: an occlusion walk ends at the first blocker it finds, the kernel's in
BVH preorder and the oracle's in index order, so either side may march instances the other never reaches (measured ratios on both
sides of 1: profiles/scene_capacity.txt).  Nor does it apply to the Cube modes, whose cell walk stops at the closest hit so far,
which depends on the visiting order.

Wall time on an MI355X: 68 tests in 3.5 s, 0.03 s or less per case but the first (context creation) and the per-frame block (0.11 s);
test_scene_capacity.py: 21 tests in 10 s on 8 CPU threads.  Every figure: profiles/scene_capacity.txt."""
import copy
import ctypes as C

import numpy as np
import pytest

import capacity_scenes as cs
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes

pytestmark = pytest.mark.gpu
TOL = 1e-4   # test_parity_gpu.py
TTOL = 1e-5  # test_ray_query_gpu.py: t relative to max(1, t), normal absolute
STAT_KEYS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits", "exhausted_rays")
EXACT_KEYS = ("primary_rays", "shadow_rays", "bounce_rays", "hits")
REF_FLAGS = _abi.FLAG_REFERENCE_VIEW_VECTOR | _abi.FLAG_REFERENCE_BOUNDARY_TEXELS
FORMS = (("one kernel", _abi.FLAG_FULL_ONE_KERNEL), ("passes", _abi.FLAG_FULL_THREE_PASS))
FORMATS = {"f32": _abi.FORMAT_F32, "texel16": _abi.FORMAT_TEXEL16}

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def leave_the_session_context_small(renderer):
    """lattice64 fills all 20 volume slots of the session's context; the modules that run later count on the high slots being
    free, as every earlier module leaves them.  A one-volume scene synced last releases slots 1 .. 19."""
    yield
    renderer.SetSceneToRender(cs.nested64("outside"))
    renderer.SyncWithScene()


def _oracle(key, sc, p):
    """One oracle frame per (scene, result-changing parameters), shared by the tests that need it (never written to)."""
    from oracle.binding import OracleScene

    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags &= REF_FLAGS
    q.path = _abi.PATH_AUTO
    full = ("frame", key, q.mode, q.max_bounces, q.flags, q.width, q.height)
    if full not in _cache:
        ref, st = OracleScene(sc).render(q, threads=8)
        ref.setflags(write=False)
        _cache[full] = (ref, st)
    return _cache[full]


def _render(r, sc, p):
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)
    img = r.Render()
    return img, r.last_timing()


def _with_flags(p, flags):
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= flags
    return q


def _check_frame(r, key, sc, p):
    """The frame in both forms: bit-equal to each other with equal counters; against the oracle as the module's docstring says."""
    ref, st = _oracle(key, sc, p)
    out = []
    for name, flag in FORMS:
        img, t = _render(r, sc, _with_flags(p, flag))
        out.append((img.copy(), {k: t[k] for k in STAT_KEYS}))
    (img, t), (img3, t3) = out
    err = np.abs(img - ref)
    ratio = [f"{t[k] / st[k]:.3f}" if st[k] else "-" for k in ("primary_steps", "shadow_steps")]  # "-": the oracle took none
    print(f"{key} mode {p.mode} path {p.path} flags {p.flags}: max |err| {err.max():.3g}, hits {t['hits']}, steps GPU / oracle: primary "
          f"{ratio[0]}, shadow {ratio[1]}")
    assert np.array_equal(img, img3), f"one kernel and passes differ in {np.count_nonzero(img != img3)} values"
    assert t == t3
    assert not np.isnan(img).any()
    assert err.max() <= TOL, f"max abs err {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
    assert {k: t[k] for k in EXACT_KEYS} == {k: st[k] for k in EXACT_KEYS}
    if p.mode < _abi.MODE_CUBE:
        assert t["primary_steps"] <= st["primary_steps"]
    return img, t


# ---- lattice64: every limit at once ------------------------------------------------------------------------------------------

LATTICE_CASES = [(f, path) for path in ("AUTO", "DENSE") for f in cs.LATTICE_FORMATS] + [("f32", "CELLS"), ("texel16", "CELLS")]


@pytest.mark.parametrize("fmt,path", LATTICE_CASES, ids=[f"{f}-{p}" for f, p in LATTICE_CASES])
def test_lattice_on_every_path_and_format(renderer, oracle_lib, fmt, path):
    """64 instances, 20 volumes, 5 + 5 lights, shadows, two bounces: fp32, texel16 and mixed (which marches the dense grids)."""
    sc = cs.lattice64(fmt)
    p = cs.params(sc, path=getattr(_abi, "PATH_" + path), bounces=2)
    _, t = _check_frame(renderer, ("lattice64", fmt), sc, p)
    assert t["bounce_rays"] > 0 and t["hits"] > 1000
    assert renderer.last_kernel_form() & _abi.FORM_FULL


@pytest.mark.parametrize("fmt", ["f32", "texel16"])
def test_lattice_in_a_cube_mode(renderer, oracle_lib, fmt):
    sc = cs.lattice64(fmt)
    _check_frame(renderer, ("lattice64", fmt), sc, cs.params(sc, mode=_abi.MODE_CUBE_NOTEX, bounces=2))


def test_lattice_of_mixed_formats_has_no_cube_kernel_and_says_so(renderer, oracle_lib):
    """VRT_ERR_UNSUPPORTED, and the context renders the next frame as it rendered the one before."""
    sc = cs.lattice64("mixed")
    p = cs.params(sc, bounces=2)
    before, _ = _render(renderer, sc, p)
    before = before.copy()
    with pytest.raises(_abi.VrtError) as e:
        _render(renderer, sc, cs.params(sc, mode=_abi.MODE_CUBE_NOTEX, bounces=2))
    assert e.value.status == _abi.VRT_ERR_UNSUPPORTED
    after, _ = _render(renderer, sc, p)
    assert np.array_equal(before, after)
    assert np.abs(after - _oracle(("lattice64", "mixed"), sc, p)[0]).max() <= TOL


def test_lattice_with_both_reference_flags(renderer, oracle_lib):
    """The REF instantiation (VRT_FLAG_REFERENCE_VIEW_VECTOR | VRT_FLAG_REFERENCE_BOUNDARY_TEXELS) of the full closest hit."""
    sc = cs.lattice64("f32")
    p = cs.params(sc, bounces=2)
    plain, _ = _check_frame(renderer, ("lattice64", "f32"), sc, p)
    img, _ = _check_frame(renderer, ("lattice64", "f32"), sc, _with_flags(p, REF_FLAGS))
    assert np.abs(img - plain).max() > 1e-5  # the flags reach the kernel


def test_lattice_as_rgba8(renderer, oracle_lib):
    """VRT_FLAG_OUTPUT_RGBA8 against the quantised oracle frame (a 1e-4 float difference can straddle a rounding boundary)."""
    from test_tiles_gloo import quantize_rgba8

    sc = cs.lattice64("f32")
    p = cs.params(sc, bounces=2)
    q = quantize_rgba8(_oracle(("lattice64", "f32"), sc, p)[0])
    imgs = [_render(renderer, sc, _with_flags(p, _abi.FLAG_OUTPUT_RGBA8 | flag))[0].copy() for _, flag in FORMS]
    assert imgs[0].dtype == np.uint8 and np.array_equal(imgs[0], imgs[1])
    d = np.abs(imgs[0].astype(np.int16) - q.astype(np.int16))
    assert d.max() <= 1 and (d != 0).mean() < 1e-2


# ---- coincident instances: the tie rule --------------------------------------------------------------------------------------

def _trace_oracle(key, sc, p, o, d, t_max):
    """OracleScene.trace of every ray (it reports the instance): hit [n] bool, t [n], normal [n, 3], instance [n] (-1: miss)."""
    from oracle.binding import OracleScene

    full = ("rays", key, p.mode)
    if full not in _cache:
        osc = OracleScene(sc)
        n = len(o)
        hit, t, nrm, inst = np.zeros(n, bool), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.full(n, -1, np.int32)
        tm = np.broadcast_to(np.asarray(t_max, np.float32), (n,))
        for k in range(n):
            h, tk, nk, ik, _ = osc.trace(p, o[k], d[k], float(tm[k]))
            if h:
                hit[k], t[k], nrm[k], inst[k] = True, tk, nk, ik
        _cache[full] = (hit, t, nrm, inst)
    return _cache[full]


def _check_closest(got, want):
    hit, t, nrm, inst = want
    assert np.array_equal(got["hit"], hit), f"{int(np.sum(got['hit'] != hit))} of {len(hit)} hit flags differ"
    assert np.array_equal(got["instance"], inst), f"{int(np.sum(got['instance'] != inst))} of {len(hit)} instances differ"
    assert np.all(np.abs(got["t"][hit] - t[hit]) <= TTOL * np.maximum(1.0, np.abs(t[hit])))
    assert np.all(np.abs(got["normal"][hit] - nrm[hit]) <= TTOL)
    assert np.all(got["t"][~hit] == -1.0) and np.all(got["normal"][~hit] == 0.0)


def _frame_rays(sc, w, h):
    from oracle.binding import OracleScene

    return OracleScene(sc).camera_rays(w, h, [(x, y) for y in range(h) for x in range(w)])


COINCIDENT_CASES = [(variant, order, fmt, mode) for variant in ("two_volumes", "pairs32") for order in (0, 1) for fmt in ("f32", "texel16")
                    for mode in ("INTERP", "CUBE")] + [("same_slot", 0, "f32", "INTERP"), ("same_slot", 0, "f32", "CUBE")] + [
                        ("shifted", order, fmt, mode) for order in (0, 1) for fmt in ("f32", "texel16") for mode in ("INTERP", "CUBE")]


@pytest.mark.parametrize("variant,order,fmt,mode", COINCIDENT_CASES, ids=["-".join(str(x) for x in c) for c in COINCIDENT_CASES])
def test_coincident_instances_show_the_lower_index(renderer, oracle_lib, variant, order, fmt, mode):
    """Twins hit at the same t: the frame shows the lower index's material (the oracle's strict '<'), and a closest-hit query reports
    the lower index exactly — in the Cube modes too, whose walk of the second twin ends AT the first one's hit.  Twins with equal boxes
    are met lower index first; "shifted" twins (bit-equal t in the Cube modes only) higher index first."""
    sc = cs.coincident(order, variant, FORMATS[fmt])
    p = cs.params(sc, mode=getattr(_abi, f"MODE_{mode}_NOTEX"))
    key = ("coincident", variant, order, fmt)
    img, t = _check_frame(renderer, key, sc, p)
    assert t["hits"] >= 100
    o, d = _frame_rays(sc, 48, 27)
    want = _trace_oracle(key, sc, p, o, d, 10000.0)
    _check_closest(renderer.trace_rays(o, d, params=p), want)
    inst = want[3][want[0]]
    assert len(inst) >= 50
    if variant == "pairs32":
        assert inst.max() < 32
    elif variant != "shifted" or mode == "CUBE":
        assert np.all(inst == 1)


# ---- equal centres, a row seen end-on, odd boxes -----------------------------------------------------------------------------

def _corner_scene(name):
    kind, *args = name.split(":")
    if kind == "nested64":
        return cs.nested64(args[0])
    if kind == "line64":
        return cs.line64(int(args[0]), args[1])
    return cs.odd_boxes(args[0])


CORNER_FRAMES = ["nested64:outside", "nested64:inside", "line64:0:along", "line64:0:back", "line64:0:diagonal", "line64:2:along",
                 "odd_boxes:near", "odd_boxes:far"]


@pytest.mark.parametrize("mode", ["INTERP", "CUBE"])
@pytest.mark.parametrize("name", CORNER_FRAMES)
def test_frames_of_the_scenes_that_corner_the_bvh(renderer, oracle_lib, name, mode):
    sc = _corner_scene(name)
    _, t = _check_frame(renderer, name, sc, cs.params(sc, mode=getattr(_abi, f"MODE_{mode}_NOTEX")))
    assert t["hits"] > 0  # (how much each scene shows: test_scene_capacity.py)


def _query_rays(name, sc):
    """About 4 000 seeded world-space rays (origins, directions, t_max per ray) for a closest-hit and an occlusion query:
    a) the camera rays of a 48x27 frame;
    b) from points in and around one instance's box towards a point in another's (around nested64's centre every origin lies in
       several boxes, many in all 64);
    c) the same with one, and with two, direction components exactly 0;
    d) origins exactly on a leaf box's lo / hi plane (the box as instance_box builds it, in float32), the direction free, lying in
       that plane (its component across the plane exactly 0: the slab's 0 * inf) or straight across it;
    e) line64: rays down the row whose t_max ends in the gap behind instance k of the row, for several k.
    A third of b) - d) get a t_max of their own between 10 and 600."""
    rng = np.random.default_rng(sum(map(ord, name)))
    lo, hi = cs.instance_boxes(sc)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    centre, half = 0.5 * (lo64 + hi64), 0.5 * (hi64 - lo64)
    n_inst = len(sc.Objects)
    o, d = _frame_rays(sc, 48, 27)
    O, D, T = [o], [d], [np.full(len(o), 10000.0, np.float32)]

    def aimed(n, spread):
        k, j = rng.integers(0, n_inst, n), rng.integers(0, n_inst, n)
        org = centre[k] + rng.uniform(-spread, spread, (n, 3)) * half[k]
        return org, centre[j] + rng.uniform(-0.8, 0.8, (n, 3)) * half[j] - org, k

    def own_t_max(n):
        t = np.full(n, 10000.0, np.float32)
        own = rng.random(n) < 1.0 / 3.0
        t[own] = rng.uniform(10.0, 600.0, int(own.sum()))
        return t

    org, dr, _ = aimed(1000, 2.5)
    O, D, T = O + [org], D + [dr], T + [own_t_max(1000)]
    for zeros in (1, 2):
        org, dr, _ = aimed(350, 2.5)
        for i in range(len(dr)):
            axes = rng.permutation(3)
            if zeros == 2:  # straight along one axis: start abreast of the target, so that the ray can meet it
                org[i, axes[:2]] += dr[i, axes[:2]]
                if dr[i, axes[2]] == 0.0:
                    dr[i, axes[2]] = 1.0
            dr[i, axes[:zeros]] = 0.0
        O, D, T = O + [org], D + [dr], T + [own_t_max(350)]
    org, dr, k = aimed(900, 1.0)
    org = org.astype(np.float32)
    for i in range(len(org)):
        a = int(rng.integers(0, 3))
        org[i, a] = (lo if rng.random() < 0.5 else hi)[k[i], a]  # exactly the float32 plane
        what = i % 3
        if what == 1:
            dr[i, a] = 0.0
        elif what == 2:
            dr[i] = 0.0
            dr[i, a] = 1.0 if rng.random() < 0.5 else -1.0
    O, D, T = O + [org], D + [dr], T + [own_t_max(900)]
    if name.startswith("line64"):
        axis = int(name.split(":")[1])
        side = [(axis + 1) % 3, (axis + 2) % 3]
        start = -31.5 * cs.LINE_PITCH - 60.0
        n = 400
        org, dr = np.zeros((n, 3)), np.zeros((n, 3))
        org[:, axis] = start
        org[:, side[0]], org[:, side[1]] = rng.uniform(-12, 12, n), rng.uniform(-12, 12, n)
        dr[:, axis] = 1.0
        tilt = np.arange(n) % 2 == 1
        dr[tilt, side[0]], dr[tilt, side[1]] = rng.uniform(-0.01, 0.01, int(tilt.sum())), rng.uniform(-0.01, 0.01, int(tilt.sum()))
        behind = np.array([0, 1, 5, 17, 31, 32, 47, 62])[rng.integers(0, 8, n)]
        O, D, T = O + [org], D + [dr], T + [((behind - 31.5) * cs.LINE_PITCH + 0.5 * cs.LINE_PITCH - start).astype(np.float32)]
    return (np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32), np.concatenate(T).astype(np.float32))


@pytest.mark.parametrize("name", ["nested64:outside", "line64:0:along", "line64:2:along", "odd_boxes:near"])
def test_ray_queries_on_the_scenes_that_corner_the_bvh(renderer, oracle_lib, name):
    """Closest hit (hit flag and instance exact, t and normal to 1e-5) and occlusion (the oracle's hit flag within t_max) of the rays
    _query_rays describes."""
    sc = _corner_scene(name)
    p = cs.params(sc)
    o, d, t_max = _query_rays(name, sc)
    assert 3500 <= len(o) <= 4500 and np.isfinite(o).all() and np.all(np.abs(d).sum(axis=1) > 0)
    zero_components = (d == 0.0).sum(axis=1)
    assert (zero_components == 1).sum() >= 300 and (zero_components == 2).sum() >= 300
    want = _trace_oracle(("queries", name), sc, p, o, d, t_max)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(p.width, p.height)
    got = renderer.trace_rays(o, d, t_max, params=p)
    print(f"{name}: {len(o)} rays, {int(want[0].sum())} hits on {len(np.unique(want[3][want[0]]))} instances")
    assert 0.1 * len(o) < want[0].sum() < 0.95 * len(o)
    _check_closest(got, want)
    occ = renderer.trace_rays(o, d, t_max, any_hit=True, params=p)
    assert np.array_equal(occ["hit"], want[0]), f"{int(np.sum(occ['hit'] != want[0]))} of {len(o)} occlusion flags differ"
    assert np.all(occ["instance"][want[0]] == 0) and np.all(occ["t"] == -1.0)


# ---- lights ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_point,n_spot", cs.LIGHT_CASES)
def test_five_point_and_five_spot_lights(renderer, oracle_lib, n_point, n_spot):
    """Every light with its own shadow bit in the passes form's hit_aux word (directional 16, point 17-21, spot 22-26); (1, 5): spot
    light 0 is not taken for point light 1."""
    sc = cs.lights(n_point, n_spot)
    _, t = _check_frame(renderer, ("lights", n_point, n_spot), sc, cs.params(sc))
    assert t["hits"] > 1000 and t["shadow_rays"] > t["hits"] * (n_point + n_spot) // 2


def test_lights_beyond_five_are_ignored(renderer, oracle_lib):
    """Seven point and seven spot light objects through VHipRenderer, and a raw vrt_scene that says n_point_lights = n_spot_lights =
    7 through vrt_scene_set and through vrt_block::scenes: each renders the (5, 5) frame bit for bit, in both forms."""
    import torch

    five, seven = cs.lights(5, 5), cs.lights(7, 7)
    p = cs.params(five)
    lib = _abi.load()
    for name, flag in FORMS:
        q = _with_flags(p, flag)
        want, t_want = _render(renderer, five, q)
        want = want.copy()
        got, t_got = _render(renderer, seven, q)
        assert np.array_equal(got, want), name
        assert {k: t_got[k] for k in STAT_KEYS} == {k: t_want[k] for k in STAT_KEYS}
        raw = (_abi.vrt_scene * 1)(five.to_abi())
        raw[0].n_point_lights = raw[0].n_spot_lights = 7
        out = torch.full((2, p.height, p.width, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        try:
            _abi.check(lib.vrt_scene_set(renderer._ctx, C.byref(raw[0])), "vrt_scene_set")
            renderer.render_rows(q, 0, p.height, out[0].data_ptr())
            torch.cuda.synchronize()
            assert {k: renderer.last_timing()[k] for k in STAT_KEYS} == {k: t_want[k] for k in STAT_KEYS}
            renderer.render_block(q, 1, out[1].data_ptr(), p.height * p.width * 16, 0, scenes=(raw, 0))
            torch.cuda.synchronize()
        finally:
            renderer.SyncWithScene()
        host = out.cpu().numpy()
        assert np.array_equal(host[0], want) and np.array_equal(host[1], want), name
    assert np.abs(want - _oracle(("lights", 5, 5), five, p)[0]).max() <= TOL


# ---- blocks of frames --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["passes", "one kernel"])
def test_a_full_frame_section_followed_by_a_nearly_empty_one(renderer, oracle_lib, form):
    """vrt_block::scenes over four frames: lattice64 (64 instances, 127 nodes, 5 + 5 lights: a full section); one instance and no
    lights; lattice64 without its last instance, 5 + 0 lights; lattice64 again.  Every frame is what vrt_scene_set(frame's scene) +
    a one-frame launch renders, bit for bit; the nearly empty frame and the last one against the oracle."""
    import torch

    base = cs.lattice64("f32")
    one, most = copy.copy(base), copy.copy(base)
    one.Objects, one.PointLights, one.SpotLights = [base.Objects[5]], [], []
    most.Objects, most.SpotLights = base.Objects[:-1], []
    frames = [base, one, most, base]
    p = _with_flags(cs.params(base, bounces=2), _abi.FLAG_FULL_ONE_KERNEL if form == "one kernel" else 0)
    n, (W, H) = len(frames), (p.width, p.height)
    # the last instance is in sight: a section that drops it renders another frame
    assert np.abs(_oracle(("lattice64", "f32"), base, p)[0] - _oracle(("lattice64", "f32", "most"), most, p)[0]).max() > 0.05
    renderer.SetSceneToRender(base)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    arr = renderer.scene_array(frames)
    block = torch.full((n, H, W, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    renderer.render_block(p, n, block.data_ptr(), H * W * 16, 0, scenes=(arr, 0))
    torch.cuda.synchronize()
    assert [fr for _, fr in renderer.launch_history(1)] == [n]
    t_block = renderer.last_timing()
    single = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    lib = _abi.load()
    try:
        for f in range(n):
            _abi.check(lib.vrt_scene_set(renderer._ctx, C.byref(arr[f])), "vrt_scene_set")
            renderer.render_rows(p, 0, H, single.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(single, block[f]), f
        assert {k: t_block[k] for k in STAT_KEYS} == {k: renderer.last_timing()[k] for k in STAT_KEYS}
    finally:
        renderer.SyncWithScene()
    host = block.cpu().numpy()
    assert not np.isnan(host).any()
    for f, key in ((1, ("lattice64", "f32", "one")), (2, ("lattice64", "f32", "most")), (3, ("lattice64", "f32"))):
        assert np.abs(host[f] - _oracle(key, frames[f], p)[0]).max() <= TOL, f
    assert np.array_equal(host[0], host[3]) and not np.array_equal(host[0], host[2])


def test_a_fused_block_of_orbit_cameras_over_the_lattice(renderer, oracle_lib):
    """Three cameras on an orbit as ONE launch: bit-equal to per-frame launches (VRT_FLAG_BLOCK_PER_FRAME), the last against the oracle."""
    import torch

    sc = cs.lattice64("f32")
    p = cs.params(sc, bounces=2)
    n, (W, H) = 3, (p.width, p.height)
    cams = scenes.orbit_cameras(sc, n, step_deg=3.0)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    fused = torch.full((n, H, W, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    single = torch.full_like(fused, float("nan"))
    renderer.render_block(p, n, fused.data_ptr(), H * W * 16, 0, cameras=cams, rows=(0, H))
    torch.cuda.synchronize()
    assert [fr for _, fr in renderer.launch_history(1)] == [n]
    t_fused = renderer.last_timing()
    renderer.render_block(_with_flags(p, _abi.FLAG_BLOCK_PER_FRAME), n, single.data_ptr(), H * W * 16, 0, cameras=cams, rows=(0, H))
    torch.cuda.synchronize()
    assert torch.equal(fused, single) and not torch.equal(fused[0], fused[n - 1])
    assert {k: t_fused[k] for k in STAT_KEYS} == {k: renderer.last_timing()[k] for k in STAT_KEYS}
    last = cs.with_camera(sc, v.VCamera(Position=cams[n - 1][0], Rotation=cams[n - 1][1], FOVAngle=cams[n - 1][2]))
    ref, st = _oracle(("lattice64", "f32", "orbit", n - 1), last, p)
    assert np.abs(fused[n - 1].cpu().numpy() - ref).max() <= TOL
    assert {k: t_fused[k] for k in EXACT_KEYS} == {k: st[k] for k in EXACT_KEYS}


def test_strips_of_the_lattice(renderer, oracle_lib):
    """vrt_render_strips (strip_rows 8, rank 1 of 3) into a sentinel-filled tile: the oracle's rows, nothing else touched."""
    import torch

    from volumetricraytracer_amd.tiles import strip_frame_rows, strip_layout

    sc = cs.lattice64("f32")
    p = cs.params(sc, bounces=2)
    W, H, world, sr, rank = p.width, p.height, 3, 8, 1
    ref, _ = _oracle(("lattice64", "f32"), sc, p)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    _, per = strip_layout(H, world, sr)
    tile = torch.full((per * sr, W, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    renderer.render_strips(p, sr, rank, world, per, tile.data_ptr())
    torch.cuda.synchronize()
    host = tile.cpu().numpy()
    touched = np.zeros(per * sr, bool)
    rays = 0
    for local0, frame0, rows in strip_frame_rows(H, world, rank, sr):
        assert not np.isnan(host[local0:local0 + rows]).any()
        assert np.abs(host[local0:local0 + rows] - ref[frame0:frame0 + rows]).max() <= TOL, frame0
        touched[local0:local0 + rows] = True
        rays += rows * W
    assert rays == 16 * W and np.isnan(host[~touched]).all()
    assert renderer.last_timing()["primary_rays"] == rays
