"""Waves that do not march (outside the cull rectangle): the batched header read, their own short path with the record stored
first, and the division-free blockIdx -> tile maps.  Yardsticks: the CPU oracle (pixels <= 1e-4, the seven counters exact) and
bit-equality between one block launch and the same frames launched one by one (VRT_FLAG_BLOCK_PER_FRAME).  Inputs: a 32^3 torus
and tiny frames — the smallest shapes at which each piece can go wrong (partial tiles in both directions, one tile, one row of
tiles, more supertiles than one XCD round, cameras in the kernarg segment and in device memory).

Not tested here: a launch with `stats` absent.  The wave's early record store is guarded by `stats != nullptr` like the store it
replaces, but no call of the C ABI can produce such a launch — every march launch binds a record buffer of its stream's slot before
it is enqueued (enqueue_rows in vrt_api.hip), and the ray-query launches, whose frame struct has no record buffer, run other
kernels — so the guard cannot be reached from a test."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from volumetricraytracer_amd import workloads as scenes
import volumetricraytracer_amd as v
from oracle.binding import OracleScene
from volumetricraytracer_amd import _abi

pytestmark = pytest.mark.gpu
TOL = 1e-4
STAT_KEYS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits", "exhausted_rays")
MAPS = {"supertile": 0, "band": 1, "linear": 2}  # vrt_params.flags bits 0-1
SIZES = [(5, 3), (16, 16), (77, 45), (1000, 8), (1920, 1080)]

_cache = {}


def _scene(kind="torus"):
    """32^3 torus; `sky`: the same scene with the camera turned away from it (empty cull rectangle: no wave marches)."""
    if kind not in _cache:
        sc = scenes.config3_torus(5, 16)
        if kind == "sky":
            sc.Camera = v.VCamera(Position=(300.0, 0.0, 40.0), Rotation=(0.0, 0.0, 0.0, 1.0), FOVAngle=60.0)
        elif kind == "inside":  # camera inside the volume's box: the rectangle is the whole frame
            sc.Camera = v.VCamera(Position=(20.0, 5.0, 60.0), Rotation=sc.Camera.Rotation, FOVAngle=60.0)
        elif kind == "corner":  # the object towards the lower right: the rectangle cuts tiles at its left and top edge
            sc.Objects[0].Position = (0.0, 95.0, -60.0)
        elif kind == "noenv":
            sc.EnvironmentMap = None
        elif kind == "bvh":
            second = copy.copy(sc.Objects[0])
            second.Position = (-40.0, 150.0, 30.0)
            sc.Objects = [sc.Objects[0], second]
        elif kind == "light":
            sc.PointLights = [v.VPointLight(Position=(150.0, 40.0, 120.0), IlluminationStrength=400.0, Color=(1.0, 0.8, 0.6, 1.0),
                                            AttenuationLinear=0.05, AttenuationExp=0.002)]
        _cache[kind] = sc
    return _cache[kind]


def _params(sc, W, H, flags=0):
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    p.flags |= flags
    return p


def _oracle(kind, W, H, flags=0):
    """One oracle frame per (scene, size, result-changing flags), shared by the tests that need it (never written to)."""
    key = ("oracle", kind, W, H, flags)
    if key not in _cache:
        sc = _scene(kind)
        ref, st = OracleScene(sc).render(_params(sc, W, H, flags), threads=8)
        ref.setflags(write=False)
        _cache[key] = (ref, st)
    return _cache[key]


def _sync(renderer, sc, W, H):
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()


def _nan_tile(rows, W):
    import torch

    return torch.full((rows, W, 4), float("nan"), dtype=torch.float32, device="cuda:0")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("tile_map", sorted(MAPS))
def test_every_pixel_is_written_once_under_every_tile_map(renderer, oracle_lib, tile_map, size):
    """Output pre-filled with a NaN sentinel: no sentinel left, every pixel the oracle's, counters exact.  1920x1080 is an all-sky
    frame (510 supertiles: more than the 8 XCDs take in one round, and no wave marches)."""
    import torch

    W, H = size
    kind = "sky" if size == (1920, 1080) else "torus"
    sc = _scene(kind)
    _sync(renderer, sc, W, H)
    p = _params(sc, W, H, MAPS[tile_map])
    out = _nan_tile(H, W)
    renderer.render_rows(p, 0, H, out.data_ptr())
    torch.cuda.synchronize()
    t = renderer.last_timing()
    img = out.cpu().numpy()
    ref, st = _oracle(kind, W, H)
    assert not np.isnan(img).any(), f"{int(np.isnan(img[..., 0]).sum())} pixels never written"
    err = np.abs(img - ref)
    print(f"{tile_map} {W}x{H}: max |err| {err.max():.3g}")
    assert err.max() <= TOL
    assert {k: t[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}
    if kind == "sky":
        assert t["primary_steps"] == 0 and t["hits"] == 0


@pytest.mark.parametrize("tile_map", sorted(MAPS))
def test_strips_and_row_ranges_off_the_tile_grid(renderer, oracle_lib, tile_map):
    """vrt_render_strips (strip_rows 8, rank 1 of 3) and a row range that starts off a tile boundary, 77x45, sentinel-filled."""
    import torch

    from volumetricraytracer_amd.tiles import strip_frame_rows, strip_layout

    W, H, world, sr, g = 77, 45, 3, 8, 1
    sc = _scene("torus")
    _sync(renderer, sc, W, H)
    p = _params(sc, W, H, MAPS[tile_map])
    ref, _ = _oracle("torus", W, H)
    _, per = strip_layout(H, world, sr)
    tile = _nan_tile(per * sr, W)
    renderer.render_strips(p, sr, g, world, per, tile.data_ptr())
    torch.cuda.synchronize()
    host = tile.cpu().numpy()
    touched = np.zeros(per * sr, bool)
    rays = 0
    for local0, frame0, rows in strip_frame_rows(H, world, g, sr):
        assert not np.isnan(host[local0:local0 + rows]).any()
        assert np.abs(host[local0:local0 + rows] - ref[frame0:frame0 + rows]).max() <= TOL
        touched[local0:local0 + rows] = True
        rays += rows * W
    assert np.isnan(host[~touched]).all()  # strip slots beyond the frame stay untouched
    assert renderer.last_timing()["primary_rays"] == rays
    row0, rows = 5, 23
    part = _nan_tile(rows, W)
    renderer.render_rows(p, row0, rows, part.data_ptr())
    torch.cuda.synchronize()
    img = part.cpu().numpy()
    assert not np.isnan(img).any()
    assert np.abs(img - ref[row0:row0 + rows]).max() <= TOL
    assert renderer.last_timing()["primary_rays"] == rows * W


def _valid_pixels_per_wave(W, H, tile_map, n_blocks):
    """Pixels of the frame inside each wave's 8x8 tile, in record order (block * 4 + wave), for a lone launch (frame 0 of a block):
    the blockIdx -> tile maps restated on the host from their description in DESIGN.md / vrt_kernels.hip."""
    tx_n, ty_n = (W + 15) // 16, (H + 15) // 16
    out = np.zeros(n_blocks * 4, np.int64)
    for b in range(n_blocks):
        xcd, q = b & 7, b >> 3
        if tile_map == "supertile":
            st, within, st_x = (q >> 4) * 8 + xcd, q & 15, (tx_n + 3) // 4
            tx, ty = (st % st_x) * 4 + (within & 3), (st // st_x) * 4 + (within >> 2)
        elif tile_map == "band":
            per, rem = n_blocks >> 3, n_blocks & 7
            L = xcd * (per + 1) + q if xcd < rem else rem * (per + 1) + (xcd - rem) * per + q
            tx, ty = L % tx_n, L // tx_n
        else:
            tx, ty = b % tx_n, b // tx_n
        if tx >= tx_n or ty >= ty_n:
            continue
        for w in range(4):
            x0, y0 = tx * 16 + (w & 1) * 8, ty * 16 + (w >> 1) * 8
            out[b * 4 + w] = max(0, min(W, x0 + 8) - x0) * max(0, min(H, y0 + 8) - y0)
    return out


@pytest.mark.parametrize("kind", ["sky", "inside", "corner"])
def test_records_of_waves_that_do_not_march(renderer, oracle_lib, kind):
    """Per-wave records (vrt_debug_wave_records) of a frame with an empty cull rectangle, one whose rectangle is the frame, and one
    whose rectangle cuts tiles at its left and top edge: primary rays sum to W x H; a wave that took no sample has the record
    {its valid pixels, 0, 0, 0, 0, 0, 0, 0}; a block's records of its first frame (the one whose blockIdx -> tile map is a lone
    launch's: the supertile map moves on by one XCD with every frame of a block) are the per-frame launch's, wave by wave."""
    import torch

    W, H, n = 77, 45, 3
    sc = _scene(kind)
    _sync(renderer, sc, W, H)
    p = _params(sc, W, H)
    out = _nan_tile(H, W)
    renderer.render_rows(p, 0, H, out.data_ptr())
    torch.cuda.synchronize()
    rec = renderer.wave_records(0)
    ref, st = _oracle(kind, W, H)
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL
    assert int(rec[:, 0].sum()) == W * H and int(rec[:, 0].max()) <= 64
    assert np.array_equal(rec[:, 0], _valid_pixels_per_wave(W, H, "supertile", rec.shape[0] // 4))  # wave by wave
    idle = rec[:, 3] == 0  # no camera-ray sample: the wave did not march (or marched rays that all missed the active box)
    assert (rec[idle, 1:] == 0).all()
    assert {k: int(rec[:, i].sum()) for i, k in enumerate(STAT_KEYS)} == {k: st[k] for k in STAT_KEYS}
    if kind == "sky":
        assert idle.all()
    else:
        assert (~idle).any() and (kind == "inside" or idle.any())
    # the frame as the first one of a block, and launched alone
    cams = [(sc.Camera.Position, sc.Camera.Rotation, 60.0)] + [(sc.Camera.Position, sc.Camera.Rotation, 50.0 + 5.0 * f) for f in range(n - 1)]
    fused = torch.zeros((n, H, W, 4), dtype=torch.float32, device="cuda:0")
    renderer.render_block(p, n, fused.data_ptr(), H * W * 16, 0, cameras=cams, rows=(0, H))
    torch.cuda.synchronize()
    block = renderer.wave_records(2)  # (of every frame of the launch)
    assert block.shape[0] == n * rec.shape[0]
    assert np.array_equal(block[:rec.shape[0]], rec)
    assert int(block[:, 0].sum()) == n * W * H
    assert torch.equal(fused[0], out)
    # ... and under the other two maps: every wave's record, marching or not, counts exactly the pixels of its own tile
    for tile_map in ("band", "linear"):
        renderer.render_rows(_params(sc, W, H, MAPS[tile_map]), 0, H, out.data_ptr())
        torch.cuda.synchronize()
        r2 = renderer.wave_records(0)
        assert np.array_equal(r2[:, 0], _valid_pixels_per_wave(W, H, tile_map, r2.shape[0] // 4)), tile_map
        assert (r2[r2[:, 3] == 0, 1:] == 0).all()
        assert {k: int(r2[:, i].sum()) for i, k in enumerate(STAT_KEYS)} == {k: st[k] for k in STAT_KEYS}


def _block_vs_per_frame(renderer, sc, p, cams, W, H, rgba8=False):
    import torch

    n = len(cams)
    dt, bpp = (torch.uint8, 4) if rgba8 else (torch.float32, 16)
    fused = torch.zeros((n, H, W, 4), dtype=dt, device="cuda:0")
    single = torch.zeros_like(fused)
    renderer.render_block(p, n, fused.data_ptr(), H * W * bpp, 0, cameras=cams, rows=(0, H))
    torch.cuda.synchronize()
    assert [fr for _, fr in renderer.launch_history(1)] == [n]
    t_fused = renderer.last_timing()
    pf = _abi.vrt_params.from_buffer_copy(p)
    pf.flags |= _abi.FLAG_BLOCK_PER_FRAME
    renderer.render_block(pf, n, single.data_ptr(), H * W * bpp, 0, cameras=cams, rows=(0, H))
    torch.cuda.synchronize()
    assert torch.equal(fused, single)
    assert {k: t_fused[k] for k in STAT_KEYS} == {k: renderer.last_timing()[k] for k in STAT_KEYS}
    return fused


def _cams(sc, n):
    """n different cameras (yaw and field of view change from frame to frame)."""
    out = []
    for f in range(n):
        a = 0.02 * f
        out.append((sc.Camera.Position, tuple(v.quat_mul(v.quat_from_axis_angle(v.UP, a), sc.Camera.Rotation)), 60.0 - 0.2 * f))
    return out


def _oracle_frame(sc, p, cam):
    sf = copy.copy(sc)
    sf.Camera = v.VCamera(Position=cam[0], Rotation=cam[1], FOVAngle=cam[2])
    return OracleScene(sf).render(p, threads=8)[0]


@pytest.mark.parametrize("n", [1, _abi.MAX_BLOCK_FRAMES, _abi.MAX_BLOCK_FRAMES + 1])
def test_blocks_with_cameras_in_the_kernarg_and_in_device_memory(renderer, oracle_lib, n):
    """Blocks of 1, MAX_BLOCK_FRAMES and MAX_BLOCK_FRAMES + 1 frames at 77x45, a camera per frame; one frame more than the kernarg
    segment holds makes the camera records come from device memory."""
    W, H = 77, 45
    sc = _scene("torus")
    _sync(renderer, sc, W, H)
    p = _params(sc, W, H)
    cams = _cams(sc, n)
    fused = _block_vs_per_frame(renderer, sc, p, cams, W, H)
    for f in sorted({0, n - 1}):
        assert np.abs(fused[f].cpu().numpy() - _oracle_frame(sc, p, cams[f])).max() <= TOL, f
    if n > 1:
        assert not np.array_equal(fused[0].cpu().numpy(), fused[n - 1].cpu().numpy())


@pytest.mark.parametrize("case", ["noenv", "rgba8", "bgra8", "ref", "bvh", "passes"])
def test_header_fields_on_every_kernel_that_reads_them(renderer, oracle_lib, case):
    """env absent, the 8-bit targets, the REF instantiation (VRT_FLAG_REFERENCE_VIEW_VECTOR), a two-instance scene (BVH kernel) and
    the passes form with one point light (primary_pass_kernel): a block of 3 frames bit-equal to per-frame launches, its last frame
    against the oracle."""
    from test_tiles_gloo import quantize_rgba8

    W, H, n = 77, 45, 3
    kind = {"noenv": "noenv", "bvh": "bvh", "passes": "light"}.get(case, "torus")
    flags = {"rgba8": _abi.FLAG_OUTPUT_RGBA8, "bgra8": _abi.FLAG_OUTPUT_RGBA8 | _abi.FLAG_OUTPUT_BGRA8,
             "ref": _abi.FLAG_REFERENCE_VIEW_VECTOR}.get(case, 0)
    sc = _scene(kind)
    _sync(renderer, sc, W, H)
    p = _params(sc, W, H, flags)
    cams = _cams(sc, n)
    eight = case in ("rgba8", "bgra8")
    fused = _block_vs_per_frame(renderer, sc, p, cams, W, H, rgba8=eight)
    form = renderer.last_kernel_form()
    if case == "passes":
        p3 = _abi.vrt_params.from_buffer_copy(p)
        renderer.render_block(p3, n, fused.data_ptr(), H * W * 16, 0, cameras=cams, rows=(0, H))
        assert renderer.last_kernel_form() & _abi.FORM_PASSES
    if case == "ref":
        assert form & _abi.FORM_LEAN_REF
    po = _abi.vrt_params.from_buffer_copy(p)
    po.flags &= ~(_abi.FLAG_OUTPUT_RGBA8 | _abi.FLAG_OUTPUT_BGRA8)
    ref = _oracle_frame(sc, po, cams[n - 1])
    img = fused[n - 1].cpu().numpy()
    if eight:
        q = quantize_rgba8(ref)
        if case == "bgra8":
            q = q[..., [2, 1, 0, 3]]
        d = np.abs(img.astype(np.int16) - q.astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() < 1e-2  # (a 1e-4 float difference can straddle a rounding boundary)
    else:
        assert np.abs(img - ref).max() <= TOL


def test_block_over_per_frame_scenes(renderer, oracle_lib):
    """A vrt_block::scenes block (the DYN instantiation: per-frame scene state and cameras in device memory): every frame is what
    vrt_scene_set(frame's scene) + a one-frame launch renders, bit for bit; the last one against the oracle."""
    import torch

    W, H, n = 77, 45, 4
    base = _scene("torus")
    frames = []
    for f in range(n):
        sc = copy.copy(base)
        o = copy.copy(base.Objects[0])
        o.Position = (0.0, 60.0 * f - 40.0, 10.0 * f)  # drifts towards the frame's edge: more and more waves outside the rectangle
        sc.Objects = [o]
        frames.append(sc)
    _sync(renderer, base, W, H)
    p = _params(base, W, H)
    arr = renderer.scene_array(frames)
    block = torch.zeros((n, H, W, 4), dtype=torch.float32, device="cuda:0")
    renderer.render_block(p, n, block.data_ptr(), H * W * 16, 0, scenes=(arr, 0))
    torch.cuda.synchronize()
    assert [fr for _, fr in renderer.launch_history(1)] == [n]
    t_block = renderer.last_timing()
    one = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    lib = _abi.load()
    try:
        for f in range(n):
            _abi.check(lib.vrt_scene_set(renderer._ctx, C.byref(arr[f])), "vrt_scene_set")
            renderer.render_rows(p, 0, H, one.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(one, block[f]), f
        assert {k: t_block[k] for k in STAT_KEYS} == {k: renderer.last_timing()[k] for k in STAT_KEYS}
    finally:
        renderer.SetSceneToRender(base)
        renderer.SyncWithScene()
    ref, _ = OracleScene(frames[n - 1]).render(p, threads=8)
    assert np.abs(block[n - 1].cpu().numpy() - ref).max() <= TOL
    assert math.isfinite(float(block.sum()))
