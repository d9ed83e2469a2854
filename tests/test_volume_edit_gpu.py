"""Incremental volume edits on the device (vrt_volume_update_region / _update_voxels): after every edit each device buffer of the
slot — dense grid, materials, bricks, cell records, both levels of the empty-space table, the Cube table and the active box — is
byte-identical to a full upload of the edited volume, so frames and counters are those of the existing contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from oracle.binding import OracleScene

pytestmark = pytest.mark.gpu
TOL = 1e-4
STAT_KEYS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits", "exhausted_rays")
WHICH = {"dense": _abi.VOLUME_BYTES_DENSE, "material": _abi.VOLUME_BYTES_MATERIAL, "bricks": _abi.VOLUME_BYTES_BRICKS,
         "cells": _abi.VOLUME_BYTES_CELLS, "skip": _abi.VOLUME_BYTES_SKIP, "nib": _abi.VOLUME_BYTES_NIB,
         "cube_skip": _abi.VOLUME_BYTES_CUBE_SKIP, "active_box": _abi.VOLUME_BYTES_ACTIVE_BOX}
EDITED, FULL = 0, 1  # slots: the edited volume, and a full upload of the same host volume


@pytest.fixture(autouse=True)
def _fresh_slots(request):
    """Tests here upload into the session renderer's slots behind SyncWithScene's back: both slots start unused (a slot keeps
    some state of its previous volume across a full upload, e.g. the active box of a volume without tables) and are freed after."""
    def free():
        if "renderer" in request.fixturenames:
            r = request.getfixturevalue("renderer")
            for slot in (EDITED, FULL):
                r._uploaded.pop(slot, None)
                r._lib.vrt_volume_free(r._ctx, slot)  # VRT_ERR_SLOT when unused
    free()
    yield
    free()


def buffers(r, slot, device=0):
    out = {}
    for name, which in WHICH.items():
        size = C.c_size_t(0)
        _abi.check(r._lib.vrt_debug_volume_bytes(r._ctx, slot, device, which, None, 0, C.byref(size)), "vrt_debug_volume_bytes")
        buf = np.zeros(size.value, np.uint8)
        _abi.check(r._lib.vrt_debug_volume_bytes(r._ctx, slot, device, which, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(size)),
                   "vrt_debug_volume_bytes")
        out[name] = buf
    return out


def assert_same_buffers(got, want, what=""):
    for name in WHICH:
        a, b = got[name], want[name]
        assert a.size == b.size, (what, name, a.size, b.size)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            pytest.fail(f"{what}: buffer {name} differs in {bad.size} of {a.size} bytes, first at byte {bad[0]}")


def make_volume(kind, res, fmt):
    vol = v.torus_volume(res, 100.0, 55.0, 22.0, v.VMaterial((0.8, 0.6, 0.2, 1.0), 0.8, 0.0))
    vol.material_id[vol.density <= 0] = 1
    if kind == "shell":  # both levels of the empty-space table live
        vol.step_max = 0.5 * vol.GetCellSize()
    return vol.set_device_format(fmt)


def update(r, slot, vol, origin, size, material=True, records=False):
    """Sends the box that vol.set_region has written: densities (+ materials), or VVoxel records."""
    (x0, y0, z0), (sx, sy, sz) = origin, size
    box = (slice(x0, x0 + sx), slice(z0, z0 + sz), slice(y0, y0 + sy))
    o, s = (C.c_int * 3)(*origin), (C.c_int * 3)(*size)
    if records:
        rec = np.zeros((sx, sz, sy), dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        rec["material"], rec["density"] = vol.material_id[box], vol.density[box]
        rc = r._lib.vrt_volume_update_voxels(r._ctx, slot, o, s, np.ascontiguousarray(rec).ctypes.data_as(C.c_void_p))
    else:
        d = np.ascontiguousarray(vol.density[box])
        m = np.ascontiguousarray(vol.material_id[box])
        rc = r._lib.vrt_volume_update_region(r._ctx, slot, o, s, d.ctypes.data_as(C.c_void_p),
                                             m.ctypes.data_as(C.c_void_p) if material else None)
    _abi.check(rc, "vrt_volume_update")
    vol.dirty_box = None


def ball(vol, center, radius_cells, sign):
    """The box around a ball of radius_cells at voxel `center` (xyz) merged into the field ([x, z, y] arrays): sign -1 adds solid,
    +1 carves."""
    n, cell = vol.N, np.float32(vol.GetCellSize())
    lo = [max(0, int(c - radius_cells - 1)) for c in center]
    hi = [min(n - 1, int(c + radius_cells + 1)) for c in center]
    x = np.arange(lo[0], hi[0] + 1)[:, None, None]
    z = np.arange(lo[2], hi[2] + 1)[None, :, None]
    y = np.arange(lo[1], hi[1] + 1)[None, None, :]
    d = (np.sqrt((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2) - radius_cells).astype(np.float32) * cell
    cur = vol.density[lo[0]:hi[0] + 1, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1]
    new = (np.minimum(cur, d) if sign < 0 else np.maximum(cur, -d)).astype(np.float32)
    return tuple(lo), new, (new <= 0).astype(np.uint8)


def edit_sequence(vol, rng):
    """(origin xyz, density [x, z, y], material [x, z, y]): random balls, a single voxel, boxes on every face, boxes from sample 4k
    to 4k + 4 (brick aprons)."""
    n = vol.N
    out = []
    for _ in range(6):
        c = rng.integers(0, n, 3)
        out.append(ball(vol, c, float(rng.uniform(1.0, max(1.5, n / 6))), int(rng.choice([-1, 1]))))
    out.append(((n // 2, n // 3, n // 4), np.full((1, 1, 1), -0.5, np.float32), np.ones((1, 1, 1), np.uint8)))
    for axis in range(3):  # boxes touching face 0 and face N-1 of every axis
        for at in (0, n - 1):
            o = [int(x) for x in rng.integers(0, max(1, n - 3), 3)]
            s = [min(3, n - x) for x in o]
            s[axis] = min(2, n)
            o[axis] = 0 if at == 0 else n - s[axis]
            d = rng.uniform(-2.0, 4.0, (s[0], s[2], s[1])).astype(np.float32)
            out.append((tuple(o), d, (d <= 0).astype(np.uint8)))
    for k in range(1, 5):
        if 4 * k + 4 >= n:
            break
        o = (4 * k, 4 * (k - 1), 4 * k)
        s = (5, 5, 5)
        d = rng.uniform(-1.0, 6.0, (s[0], s[2], s[1])).astype(np.float32)
        out.append((o, d, (d <= 0).astype(np.uint8)))
    return out


def run_sequence(r, vol, rng, records_every=5):
    for slot in (EDITED, FULL):
        r._lib.vrt_volume_free(r._ctx, slot)
    r.upload_volume(EDITED, vol)
    for i, (o, d, m) in enumerate(edit_sequence(vol, rng)):
        vol.set_region(o, d, m)
        size = (d.shape[0], d.shape[2], d.shape[1])
        update(r, EDITED, vol, o, size, records=(i % records_every == records_every - 1))
        r.upload_volume(FULL, vol)
        assert_same_buffers(buffers(r, EDITED), buffers(r, FULL), f"edit {i} at {o} size {size}")


@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
@pytest.mark.parametrize("kind", ["torus", "shell"])
def test_every_buffer_equals_a_full_upload_after_each_edit(renderer, fmt, kind):
    rng = np.random.default_rng(11 + fmt + 2 * (kind == "shell"))
    vol = make_volume(kind, 6, fmt)
    run_sequence(renderer, vol, rng)
    n = vol.N
    # no materials sent: the box keeps its own
    before = vol.material_id[4:7, 4:7, 4:7].copy()
    vol.set_region((4, 4, 4), np.full((3, 3, 3), -0.25, np.float32))
    update(renderer, EDITED, vol, (4, 4, 4), (3, 3, 3), material=False)
    assert np.array_equal(vol.material_id[4:7, 4:7, 4:7], before)
    renderer.upload_volume(FULL, vol)
    assert_same_buffers(buffers(renderer, EDITED), buffers(renderer, FULL), "no materials")
    # every active cell removed: no near brick, an empty active box, a Cube table without a seed
    empty = lambda: (np.full((n, n, n), 30.0, np.float32), np.zeros((n, n, n), np.uint8))
    vol.set_region((0, 0, 0), *empty())
    update(renderer, EDITED, vol, (0, 0, 0), (n, n, n))
    renderer.upload_volume(FULL, vol)
    got = buffers(renderer, EDITED)
    assert_same_buffers(got, buffers(renderer, FULL), "all removed")
    assert (got["cube_skip"] == 255).all()
    if kind == "shell":
        assert (got["skip"] == 254).all()  # the leap count of "no near brick" (distance 255 - 1)
        assert list(got["active_box"].view(np.int32)) == [(n - 1) // 4] * 3 + [-1] * 3
    # lone active cells 15, 16, 17 and 40 cells from any other: the edges of the level-2 table's 16-cell window
    for gap in (15, 16, 17, 40):
        vol.set_region((0, 0, 0), *empty())
        update(renderer, EDITED, vol, (0, 0, 0), (n, n, n))
        for p in ((3, 5, 7), (3 + gap, 5, 7), (3 + gap, 5 + gap, 7), (3, 5, 7 + gap)):
            if max(p) >= n:
                continue
            vol.set_region(p, np.full((1, 1, 1), -0.3, np.float32), np.ones((1, 1, 1), np.uint8))
            update(renderer, EDITED, vol, p, (1, 1, 1))
            renderer.upload_volume(FULL, vol)
            assert_same_buffers(buffers(renderer, EDITED), buffers(renderer, FULL), f"gap {gap} at {p}")
    # the whole volume as one box
    fresh = make_volume(kind, 6, fmt)
    vol.set_region((0, 0, 0), fresh.density, fresh.material_id)
    update(renderer, EDITED, vol, (0, 0, 0), (n, n, n), records=True)
    renderer.upload_volume(FULL, vol)
    assert_same_buffers(buffers(renderer, EDITED), buffers(renderer, FULL), "whole volume")


@pytest.mark.parametrize("res", [0, 1, 2])
@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
def test_small_resolutions(renderer, res, fmt):
    rng = np.random.default_rng(100 + res)
    for kind in ("torus", "shell"):
        run_sequence(renderer, make_volume(kind, res, fmt), rng, records_every=3)


def test_a_256_cubed_shell_with_a_few_edits(renderer):
    vol = scenes.voxelized_torus(8).set_device_format(_abi.FORMAT_TEXEL16)
    assert vol.N == 257 and vol.step_max > 0
    renderer.upload_volume(EDITED, vol)
    for i, (c, rad, sign) in enumerate((((128, 128, 200), 10.0, 1), ((60, 130, 128), 20.0, -1), ((0, 255, 256), 6.0, -1))):
        o, d, m = ball(vol, c, rad, sign)
        vol.set_region(o, d, m)
        update(renderer, EDITED, vol, o, (d.shape[0], d.shape[2], d.shape[1]), records=(i == 1))
    renderer.upload_volume(FULL, vol)
    assert_same_buffers(buffers(renderer, EDITED), buffers(renderer, FULL), "256^3")


def edited_scene(fmt):
    sc = scenes.config3_torus(6, 16)
    vol = sc.volumes()[0].set_device_format(fmt)
    vol.step_max = 0.5 * vol.GetCellSize()
    return sc, vol


def carve(vol):
    """Edits the side of the torus (ring around z, 17.6 cells out, tube 7 cells) that faces the camera: two bites, one lump."""
    for c, rad, sign in (((50, 32, 40), 5.0, 1), ((57, 32, 32), 4.0, 1), ((32, 50, 40), 4.0, -1)):
        vol.set_region(*ball(vol, c, rad, sign))


@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
def test_frames_after_edits(oracle_lib, fmt):
    sc, vol = edited_scene(fmt)
    cell = scenes.min_cell(sc)
    paths = (_abi.PATH_DENSE, _abi.PATH_BRICK, _abi.PATH_AUTO) + ((_abi.PATH_CELLS,) if fmt == _abi.FORMAT_TEXEL16 else ())
    cases = [(path, mode, False) for mode in (_abi.MODE_INTERP_NOTEX, _abi.MODE_CUBE_NOTEX) for path in paths]
    cases.append((_abi.PATH_AUTO, _abi.MODE_INTERP_NOTEX, True))
    with v.VHipRenderer() as r:
        r.SetSceneToRender(sc)
        r.SyncWithScene()
        carve(vol)
        assert vol.dirty_box is not None and not vol.dirty
        edited = []
        for path, mode, shadow in cases:
            p = v.default_params(256, 144, cell, 255, shadow=shadow, mode=mode, path=path)
            r.ResizeRenderOutput(p.width, p.height)
            r.params_override = p
            r.SetRendererMode(mode)
            img = r.Render()  # the first one's sync sends the box (vrt_volume_update_region)
            assert vol.dirty_box is None
            t = r.last_timing()
            ref, st = OracleScene(sc).render(p, threads=8)
            assert np.abs(img - ref).max() <= TOL, (path, mode, shadow)
            assert {k: t[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, (path, mode, shadow)
            assert t["hits"] > 0
            edited.append(img)
        vol.dirty = True  # the whole volume uploaded again
        for (path, mode, shadow), img in zip(cases, edited):
            p = v.default_params(256, 144, cell, 255, shadow=shadow, mode=mode, path=path)
            r.params_override = p
            r.SetRendererMode(mode)
            assert np.array_equal(r.Render(), img), (path, mode, shadow)


def _frame_renderer(r, sc, p):
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)


def test_a_frame_begun_before_an_edit_renders_the_old_volume(oracle_lib):
    sc, vol = edited_scene(_abi.FORMAT_F32)
    p = v.default_params(256, 144, scenes.min_cell(sc), 255, shadow=True)
    with v.VHipRenderer() as r:
        _frame_renderer(r, sc, p)
        before = r.Render()
        r.render_begin(0, p)
        carve(vol)
        r.render_begin(1, p)  # its sync sends the box once the frame on slot 0 is done
        first, second = r.render_end(0, p), r.render_end(1, p)
        after = r.Render()
    assert np.array_equal(first, before)
    assert np.array_equal(second, after)
    assert not np.array_equal(before, after)


def test_a_context_over_two_devices_updates_both(oracle_lib):
    frames = []
    for devices in ((0, 0), (0,)):
        sc, vol = edited_scene(_abi.FORMAT_TEXEL16)
        p = v.default_params(256, 144, scenes.min_cell(sc), 255, shadow=True)
        with v.VHipRenderer(devices=devices) as r:
            _frame_renderer(r, sc, p)
            r.Render()
            carve(vol)
            frames.append(r.Render())
            if len(devices) == 2:
                r.upload_volume(FULL, vol)
                want = buffers(r, FULL)
                for dev in (0, 1):
                    assert_same_buffers(buffers(r, EDITED, dev), want, f"device {dev}")
    assert np.array_equal(frames[0], frames[1])


def test_refused_calls_change_nothing(renderer):
    vol = make_volume("shell", 5, _abi.FORMAT_TEXEL16)
    renderer.upload_volume(EDITED, vol)
    before = buffers(renderer, EDITED)
    lib, ctx, n = renderer._lib, renderer._ctx, vol.N
    d = np.zeros(8 * n ** 3, np.float32)
    ptr = d.ctypes.data_as(C.c_void_p)
    box = lambda *a: (C.c_int * 3)(*a)
    assert lib.vrt_volume_update_region(ctx, 7, box(0, 0, 0), box(1, 1, 1), ptr, None) == _abi.VRT_ERR_SLOT
    assert lib.vrt_volume_update_voxels(ctx, _abi.VRT_MAX_VOLUMES, box(0, 0, 0), box(1, 1, 1), ptr) == _abi.VRT_ERR_SLOT
    for o, s in (((0, 0, 0), (n + 1, 1, 1)), ((n - 1, 0, 0), (2, 1, 1)), ((0, -1, 0), (1, 1, 1)), ((0, 0, n), (1, 1, 1)),
                 ((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, 1, -3))):
        assert lib.vrt_volume_update_region(ctx, EDITED, box(*o), box(*s), ptr, None) == _abi.VRT_ERR_INVALID, (o, s)
        assert lib.vrt_volume_update_voxels(ctx, EDITED, box(*o), box(*s), ptr) == _abi.VRT_ERR_INVALID, (o, s)
    assert lib.vrt_volume_update_region(ctx, EDITED, box(0, 0, 0), box(1, 1, 1), None, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_update_voxels(ctx, EDITED, box(0, 0, 0), box(1, 1, 1), None) == _abi.VRT_ERR_INVALID
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")


def test_a_captured_frame_replays_over_the_edited_volume(renderer, oracle_lib):
    """Device pointers survive an edit: a render_rows launch captured before it replays the edited volume."""
    import torch

    sc, vol = edited_scene(_abi.FORMAT_F32)
    p = v.default_params(200, 120, scenes.min_cell(sc), 255, shadow=True)
    p.flags |= _abi.FLAG_NO_CULL_RECT  # a captured launch keeps its cull rectangle, and an edit may grow the active box
    renderer.SetSceneToRender(sc)
    renderer.SyncWithScene()
    side = torch.cuda.Stream()
    out = torch.zeros((120, 200, 4), dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(side):
        renderer.render_rows(p, 0, 120, out.data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    old = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        renderer.render_rows(p, 0, 120, out.data_ptr(), side.cuda_stream)
    carve(vol)
    renderer.SyncWithScene()
    assert vol.dirty_box is None
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    fresh = torch.zeros_like(out)
    renderer.render_rows(p, 0, 120, fresh.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out, fresh) and not torch.equal(out, old)
    ref, _ = OracleScene(sc).render(p, threads=8)
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL
    got = renderer.download_volume(0, vol.Resolution, vol.VolumeExtends)
    assert np.array_equal(got.density, vol.density) and np.array_equal(got.material_id, vol.material_id)


def test_cpp_adaptor_region_updates_render_what_full_uploads_render(tmp_path):
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    outs = {}
    for name, extra in (("region", ["--edit-brush", "6"]), ("full", ["--edit-brush", "6", "--edit-full"]), ("plain", [])):
        out = str(tmp_path / (name + ".ppm"))
        r = subprocess.run([exe, "--frames", "10", "--size", "320x180", "--out", out] + extra, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr
        outs[name] = open(out, "rb").read()
        if name != "plain":
            assert ("region updates" if name == "region" else "full uploads") in r.stdout
    assert outs["region"] == outs["full"]
    assert outs["region"] != outs["plain"]  # the brush changed the frame
