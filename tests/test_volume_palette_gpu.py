"""Per-voxel materials on the GPU (vrt_volume_set_palette): a palette of equal entries renders what the slot's material renders; on the
painted sphere (tests/palette_ref.py) every hit pixel of the palette frame is, bit for bit, the pixel of the frame rendered with that
hit's entry as the whole slot's material — the entry named by the numpy restatement of the header's rule from the GPU's own closest
hit — also through a block of frames with per-frame scenes, behind a mirror bounce and in a textured mode; ids beyond the palette keep
the slot's material; the palette comes and goes without a trace, follows undo, and bad arguments change nothing.  Pixels nearer than
palette_ref.MARGIN_CELLS to a place where the rule's decision changes are left out (the device rounds the hit point in fp32), and
their share is capped.  The helpers these tests share with tests/test_volume_palette_paths_gpu.py live in tests/palette_ref.py; that
suite runs the same comparison on every kernel path (the Cube modes among them) with and without per-frame scenes, on slots and instances
whose numbers differ, with two palettes, where only an entry or only the slot mirrors, under a roughness / metallic texture, on two
devices, on -0 / +0 samples with id 255, and on many hits without an INSIDE corner."""
import ctypes as C

import numpy as np
import pytest

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

import brush_ref
import palette_ref as pr
from palette_ref import bits, camera_hits, check_composition, frame, material_of, uniform_frames, use
from volume_ref import F32

pytestmark = pytest.mark.gpu
ONE = _abi.FLAG_FULL_ONE_KERNEL
COUNTERS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits")


@pytest.fixture(scope="module")
def pal(oracle_lib):
    """A context of this module's own."""
    with v.VHipRenderer() as r:
        yield r


def painted(r, fmt=_abi.FORMAT_F32, mirror=False, mode=_abi.MODE_INTERP_NOTEX, max_bounces=0, texture=None):
    """The painted sphere on the device (slot 0), painted there by the PAINT record; returns (scene, params, volume)."""
    vol = pr.sphere_volume(fmt)
    vol.Material = material_of(pr.ENTRIES[0])
    if texture is not None:
        vol.Material.AlbedoTexture = texture
        vol.Material.TextureScale = (7.0, 5.0)
    sc = pr.painted_sphere_scene(vol, pr.mirror_volume() if mirror else None, yaw=pr.MIRROR_SPHERE_YAW if mirror else 0.35)
    p = pr.scene_params(sc, mode=mode, flags=ONE, max_bounces=max_bounces)
    use(r, sc, p)
    res = r.apply_brushes(0, vol, [pr.paint_record()])
    assert res["written"] > 0 and set(np.unique(vol.material_id)) == {0, 1, 2}
    return sc, p, vol


def entry_of_hits(r, sc, rays, got, which):
    """ids and boundary distances of the hits `which` (a mask over the pixels) on instance 0, from the volume as the device holds it."""
    dv = r.download_volume(0, pr.RESOLUTION, pr.EXTENT)
    obj = sc.Objects[0]
    pts = pr.object_points(obj.Position, obj.Rotation, obj.Scale, rays["origin"][which], rays["direction"][which], got["t"][which])
    return pr.entry_ids(dv.density, dv.material_id, pr.EXTENT, pts)


# ---- 1. a palette of equal entries is the material ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
@pytest.mark.parametrize("path", [_abi.PATH_BRICK, _abi.PATH_CELLS, _abi.PATH_DENSE])
def test_uniform_palette_equals_material(pal, fmt, path):
    r = pal
    M = ((0.7, 0.5, 0.2, 1.0), 0.2, 0.4)  # roughness 0.2: it mirrors
    vol = pr.sphere_volume(fmt)
    vol.Material = material_of(M)
    objs = [v.VVoxelObject(Position=(-13.0, 0.0, 0.0), Rotation=tuple(v.quat_from_axis_angle(v.UP, 0.35)), Scale=(1.1, 1.0, 0.9), Volume=vol),
            v.VVoxelObject(Position=(13.0, 2.0, 1.0), Volume=vol)]
    base = pr.painted_sphere_scene(vol)
    point = v.VPointLight(Position=(0.0, 30.0, 20.0), IlluminationStrength=300.0, Color=(1.0, 0.9, 0.7, 1.0), AttenuationLinear=0.05,
                          AttenuationExp=0.002)
    sc = v.VScene(Camera=base.Camera, DirectionalLight=base.DirectionalLight, Objects=objs, PointLights=[point],
                  EnvironmentMap=base.EnvironmentMap)
    p = pr.scene_params(sc, path=path, flags=ONE, max_bounces=2)
    use(r, sc, p)
    r.apply_brushes(0, vol, [pr.paint_record()])  # ids 0, 1 and 2 on the device: every one of them must land on M
    A, tA, fA = frame(r)
    r.set_palette(0, [M] * 256)
    B, tB, fB = frame(r)
    worst = float(np.abs(A - B).max())
    print(f"fmt {fmt} path {path}: max |B - A| = {worst:.3e}, bit for bit: {np.array_equal(bits(A), bits(B))}, bounce rays {tA['bounce_rays']}")
    assert worst <= 1e-4  # the parity tolerance of tests/test_parity_gpu.py; expected: 0
    assert np.array_equal(bits(A), bits(B))
    for k in COUNTERS:
        assert tA[k] == tB[k], k
    assert tA["bounce_rays"] > 0 and tA["hits"] > 0
    assert fA & _abi.FORM_FULL and not fA & _abi.FORM_PALETTE
    assert fB & _abi.FORM_FULL and fB & _abi.FORM_PALETTE and not fB & _abi.FORM_PASSES


# ---- 2. per-pixel composition ------------------------------------------------------------------------------------------------------
def test_per_pixel_composition_and_a_block_of_frames_with_their_own_scenes(pal):
    import torch

    r = pal
    sc, p, vol = painted(r)
    ref_m = pr.sphere_volume().material_id.copy()
    ref_d = pr.sphere_volume().density.copy()
    brush_ref.apply(ref_d, ref_m, F32, [pr.paint_record()], pr.EXTENT, 1.0)
    assert np.array_equal(vol.material_id, ref_m)  # the device painted what the restatement paints
    U = uniform_frames(r, vol, pr.ENTRIES)
    r.set_palette(0, pr.ENTRIES)
    P, _, form = frame(r)
    assert form & _abi.FORM_FULL and form & _abi.FORM_PALETTE and not form & _abi.FORM_PASSES
    rays, got = camera_hits(r, p)
    hit = got["hit"]
    ids, dist = entry_of_hits(r, sc, rays, got, hit)
    check_composition(P, U, ids, dist, np.flatnonzero(hit), int(hit.sum()))
    sky = ~hit
    for k in range(3):
        assert np.array_equal(bits(P).reshape(-1, 4)[sky], bits(U[k]).reshape(-1, 4)[sky])
    assert np.any(bits(U[1]) != bits(U[2]))
    # the same through vrt_render_block: three frames with their own scenes (the DYN instantiation), one launch, one kernel
    moved = pr.painted_sphere_scene(vol)
    moved.Objects[0].Position = (3.0, 0.0, -0.5)
    arr = r.scene_array([sc, moved, sc])
    out = torch.zeros((3, p.height, p.width, 4), dtype=torch.float32, device="cuda")
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags = 0  # no VRT_FLAG_FULL_ONE_KERNEL: a palette alone keeps the block in one kernel
    r.render_block(q, 3, out.data_ptr(), p.height * p.width * 16, 0, scenes=(arr, 0))
    torch.cuda.synchronize()
    form = r.last_kernel_form()
    assert form & _abi.FORM_FULL and form & _abi.FORM_PALETTE and not form & _abi.FORM_PASSES
    assert r.launch_history(1)[-1][1] == 3  # one launch covered the three frames
    blk = out.cpu().numpy()
    assert np.array_equal(bits(blk[0]), bits(P)) and np.array_equal(bits(blk[2]), bits(P))
    assert np.any(bits(blk[1]) != bits(P))  # the frame's own scene was rendered
    q.flags = _abi.FLAG_FULL_THREE_PASS
    b = _abi.vrt_block()
    b.n_frames, b.rows, b.frame_stride_bytes = 3, p.height, p.height * p.width * 16
    b.scenes = C.cast(arr, C.POINTER(_abi.vrt_scene))
    assert r._lib.vrt_render_block(r._ctx, C.byref(q), C.byref(b), C.c_void_p(out.data_ptr()), None) == _abi.VRT_ERR_UNSUPPORTED


# ---- 3. behind a mirror bounce -----------------------------------------------------------------------------------------------------
def test_the_mirror_level_takes_the_palette_too(pal):
    r = pal
    sc, p, vol = painted(r, mirror=True, max_bounces=1)
    U = uniform_frames(r, vol, pr.ENTRIES)
    # (entry 0 = entry 1: the rare hit in a cell without an INSIDE corner, whose nearest sample carries id 0, then shows entry 1 too)
    r.set_palette(0, (pr.ENTRIES[1], pr.ENTRIES[1], pr.ENTRIES[2]))
    P, t, form = frame(r)
    assert form & _abi.FORM_PALETTE and form & _abi.FORM_MAY_BOUNCE and t["bounce_rays"] > 0
    _, got = camera_hits(r, p)
    mirror = (got["hit"] & (got["instance"] == 1))
    Pb, U1, U2 = bits(P).reshape(-1, 4), bits(U[1]).reshape(-1, 4), bits(U[2]).reshape(-1, 4)
    differ = mirror & np.any(U1 != U2, axis=1)  # the mirror shows the sphere there
    is1, is2 = np.all(Pb == U1, axis=1), np.all(Pb == U2, axis=1)
    print(f"mirror pixels {int(mirror.sum())}, showing the sphere {int(differ.sum())}: entry 1 {int((differ & is1).sum())}, "
          f"entry 2 {int((differ & is2).sum())}, neither {int((differ & ~is1 & ~is2).sum())}")
    assert int(differ.sum()) > 50
    assert np.all((is1 | is2)[differ])
    assert np.any((is1 & ~is2)[differ]) and np.any((is2 & ~is1)[differ])


# ---- 4. fallback and lifetime ------------------------------------------------------------------------------------------------------
def test_ids_beyond_the_palette_and_the_palettes_lifetime(pal):
    r = pal
    sc, p, vol = painted(r)
    slot_m = ((0.3, 0.8, 0.4, 1.0), 0.6, 0.2)
    vol.Material = material_of(slot_m)
    U = uniform_frames(r, vol, (pr.ENTRIES[0], pr.ENTRIES[1], slot_m))  # id 2 is beyond a palette of two: the slot's own material
    base, _, _ = frame(r)
    r.set_palette(0, pr.ENTRIES[:2])
    P, _, form = frame(r)
    assert form & _abi.FORM_PALETTE
    rays, got = camera_hits(r, p)
    hit = got["hit"]
    ids, dist = entry_of_hits(r, sc, rays, got, hit)
    check_composition(P, U, ids, dist, np.flatnonzero(hit), int(hit.sum()))
    # get round-trips, bit for bit
    back = r.get_palette(0)
    want = np.array([list(e[0]) + [e[1], e[2]] for e in pr.ENTRIES[:2]], np.float32)
    assert back.shape == (2, 6) and np.array_equal(back.view(np.uint32), want.view(np.uint32))
    n = C.c_int(-1)
    one = (_abi.vrt_material * 1)()
    assert r._lib.vrt_volume_get_palette(r._ctx, 0, 1, one, C.byref(n)) == _abi.VRT_ERR_INVALID and n.value == 2
    # the argument errors: each returns its code and leaves the frame as it was
    lib, ctx = r._lib, r._ctx
    two = (_abi.vrt_material * 2)()
    for m in two:
        m.tint[:] = (0.5, 0.5, 0.5, 1.0)
        m.roughness, m.metallic = 0.5, 0.0
    bad = (_abi.vrt_material * 2)(two[0], two[1])
    bad[1].metallic = float("nan")
    inf = (_abi.vrt_material * 2)(two[0], two[1])
    inf[0].tint[2] = float("inf")
    assert lib.vrt_volume_set_palette(None, 0, 2, two) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_set_palette(ctx, 0, -1, two) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_set_palette(ctx, 0, 257, two) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_set_palette(ctx, 0, 2, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_set_palette(ctx, 0, 2, bad) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_set_palette(ctx, 0, 2, inf) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_set_palette(ctx, 7, 2, two) == _abi.VRT_ERR_SLOT
    assert lib.vrt_volume_get_palette(ctx, 7, 2, two, C.byref(n)) == _abi.VRT_ERR_SLOT
    again, _, _ = frame(r)
    assert np.array_equal(bits(again), bits(P)) and len(r.get_palette(0)) == 2
    # the three passes have no palette: refused before anything changes
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags = _abi.FLAG_FULL_THREE_PASS
    img = np.zeros((p.height, p.width, 4), np.float32)
    assert lib.vrt_render(ctx, C.byref(q), img.ctypes.data_as(C.c_void_p)) == _abi.VRT_ERR_UNSUPPORTED
    again, _, _ = frame(r)
    assert np.array_equal(bits(again), bits(P))
    # a PAINT dab and its undo
    r.enable_history(0, 8, 1 << 20)
    N = vol.N
    dab = v.sphere_brush(_abi.BRUSH_PAINT, (0.5 * (N - 1), N - 6.0, 0.5 * (N - 1)), 5.0, material=0)  # on the side the camera sees
    assert r.apply_brushes(0, vol, [dab])["written"] > 0
    dabbed, _, _ = frame(r)
    assert np.any(bits(dabbed) != bits(P))
    assert r.undo(0, 1, vol)["written"] > 0
    undone, _, _ = frame(r)
    assert np.array_equal(bits(undone), bits(P))
    assert len(r.get_palette(0)) == 2  # neither recorded nor undone
    r.enable_history(0, 0, 0)
    # n = 0 takes it away: the frame from before the palette, bit for bit
    r.set_palette(0, None)
    off, _, form = frame(r)
    assert np.array_equal(bits(off), bits(base)) and not form & _abi.FORM_PALETTE and len(r.get_palette(0)) == 0
    # ... and the lean kernel again in a lean scene (no spot light), which a palette alone turns into a full closest hit
    lean = pr.painted_sphere_scene(vol)
    lean.SpotLights = []
    q = pr.scene_params(lean)
    use(r, lean, q)
    a, _, form = frame(r)
    assert not form & (_abi.FORM_FULL | _abi.FORM_PALETTE)
    r.set_palette(0, [slot_m] * 3)
    b, _, form = frame(r)
    assert form & _abi.FORM_FULL and form & _abi.FORM_PALETTE and not form & _abi.FORM_PASSES
    print(f"lean frame against the same frame through a palette of the slot's own material: max |diff| = {float(np.abs(a - b).max()):.3e}")
    r.set_palette(0, None)
    c, _, form = frame(r)
    assert np.array_equal(bits(c), bits(a)) and not form & (_abi.FORM_FULL | _abi.FORM_PALETTE)
    # a fresh upload into the used slot keeps the palette, vrt_volume_free drops it
    r.set_palette(0, pr.ENTRIES)
    vol.dirty = True
    r.SyncWithScene()
    assert len(r.get_palette(0)) == 3
    r.set_palette(0, None)


# ---- 5. a textured mode ------------------------------------------------------------------------------------------------------------
def test_composition_in_a_textured_mode(pal):
    r = pal
    tex = np.array([[[255, 255, 255, 255], [60, 200, 90, 255]], [[200, 80, 220, 255], [30, 30, 160, 255]]], np.uint8)  # 2 x 2 albedo
    sc, p, vol = painted(r, mode=_abi.MODE_INTERP, texture=tex)
    U = uniform_frames(r, vol, pr.ENTRIES)
    r.set_palette(0, pr.ENTRIES)
    P, _, form = frame(r)
    assert form & _abi.FORM_PALETTE and form & _abi.FORM_TEXTURED
    rays, got = camera_hits(r, p)
    hit = got["hit"]
    ids, dist = entry_of_hits(r, sc, rays, got, hit)
    check_composition(P, U, ids, dist, np.flatnonzero(hit), int(hit.sum()))
    r.set_palette(0, None)
