"""Enclosed-cavity fill on the device (vrt_volume_fill_enclosed): after the call each device buffer of the slot — dense grid, materials,
bricks, cell records, both levels of the empty-space table, the Cube table and the active box — is byte-identical to the numpy
reference of the contract (tests/fill_ref.py) pushed through the reference of the upload (tests/volume_ref.py), and to a full upload
of that field; so frames and counters are those of the existing contract."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import brush_ref as B
import fill_ref as F
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx
from volumetricraytracer_amd import workloads as scenes
from oracle.binding import OracleScene

pytestmark = pytest.mark.gpu
TOL = 1e-4
STAT_KEYS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits", "exhausted_rays")
WHICH = {"dense": _abi.VOLUME_BYTES_DENSE, "material": _abi.VOLUME_BYTES_MATERIAL, "bricks": _abi.VOLUME_BYTES_BRICKS,
         "cells": _abi.VOLUME_BYTES_CELLS, "skip": _abi.VOLUME_BYTES_SKIP, "nib": _abi.VOLUME_BYTES_NIB,
         "cube_skip": _abi.VOLUME_BYTES_CUBE_SKIP, "active_box": _abi.VOLUME_BYTES_ACTIVE_BOX}
EDITED, FULL = 0, 1  # slots: the filled volume, and a full upload of the reference's field
FORMATS = [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16]


@pytest.fixture(autouse=True)
def _fresh_slots(request):
    """Tests here upload into the session renderer's slots behind SyncWithScene's back: both slots start unused and are freed after."""
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
    """Tolerance 0.  A reference entry that is None (the active box of a slot without tables) is not compared."""
    for name in WHICH:
        a, b = got[name], want[name]
        if b is None:
            continue
        assert a.size == b.size, (what, name, a.size, b.size)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            pytest.fail(f"{what}: buffer {name} differs in {bad.size} of {a.size} bytes, first at byte {bad[0]}")


class Case:
    """A volume, what the device stores for it (DENSE field and material ids), and the reference's fill of that — computed once per
    (volume, format) and never written to afterwards."""

    def __init__(self, vol, wall, material):
        self.vol, self.fmt, self.wall, self.material_id = vol, int(vol.device_format), wall, material
        self.stored = R.dense_field(np.array(vol.density, np.float32), self.fmt)
        self.material = np.array(vol.material_id, np.uint8)
        self.want_d, self.want_m, self.info = F.fill(self.stored, self.material, self.fmt, wall, material)
        for a in (self.stored, self.material, self.want_d, self.want_m):
            a.setflags(write=False)

    def device_bytes(self, stored=None, material=None):
        stored = self.want_d if stored is None else stored
        material = self.want_m if material is None else material
        return R.device_bytes(stored, material, self.fmt, self.vol.density_scale, self.vol.step_max)


def upload_field(r, slot, vol, fmt, stored, material):
    """A full upload of exactly this stored field: the floats (F32), or the RGBA8 texels of +-q (TEXEL16 — uploading q * 0.01 as floats
    would quantise a second time)."""
    lib, ctx = r._lib, r._ctx
    if fmt == _abi.FORMAT_F32:
        _abi.check(lib.vrt_set_volume_format(ctx, _abi.FORMAT_F32), "vrt_set_volume_format")
        d, m = np.ascontiguousarray(stored), np.ascontiguousarray(material)
        rc = lib.vrt_volume_upload(ctx, slot, vol.Resolution, vol.VolumeExtends, d.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p))
    else:
        tex = B.texels_of(stored, material)
        rc = lib.vrt_volume_upload_texels(ctx, slot, vol.Resolution, vol.VolumeExtends, tex.ctypes.data_as(C.c_void_p))
    _abi.check(rc, "vrt_volume_upload*")
    _abi.check(lib.vrt_volume_set_metric(ctx, slot, float(vol.density_scale), float(vol.step_max)), "vrt_volume_set_metric")


def check_result(got, want, what):
    assert got["filled"] == want["filled"], (what, got, want)
    if want["filled"] == 0:
        assert all(l > h for l, h in zip(got["lo"], got["hi"])), (what, got)
    else:
        assert got["lo"] == want["lo"] and got["hi"] == want["hi"], (what, got, want)


def fill_and_check(r, case, what):
    """Upload into EDITED, one call, every buffer against both witnesses; then a second call, which must change nothing."""
    vol = case.vol
    upload_field(r, EDITED, vol, case.fmt, case.stored, case.material)
    before = buffers(r, EDITED)
    got = r.fill_enclosed(EDITED, None, case.wall, case.material_id)
    print(f"{what}: filled {got['filled']} (reference {case.info['filled']}), box {got['lo']}..{got['hi']}, {got['sweeps']} device rounds, "
          f"{case.info['sweeps']} dilation sweeps")
    check_result(got, case.info, what)
    have = buffers(r, EDITED)
    assert_same_buffers(have, case.device_bytes(), what + " against the reference")
    upload_field(r, FULL, vol, case.fmt, case.want_d, case.want_m)
    assert_same_buffers(have, buffers(r, FULL), what + " against a full upload")
    if case.info["filled"] == 0:
        assert_same_buffers(have, before, what + ": nothing to fill, nothing changed")
    again = r.fill_enclosed(EDITED, None, case.wall, case.material_id)
    assert again["filled"] == 0 and all(l > h for l, h in zip(again["lo"], again["hi"])), (what, again)
    assert_same_buffers(buffers(r, EDITED), have, what + " after a second call")
    return got


@functools.lru_cache(maxsize=None)
def shell(res):
    return scenes.voxelized_torus(res)


@functools.lru_cache(maxsize=None)
def volume_case(name, fmt):
    if name == "sdf":  # a true SDF, solid inside, without the empty-space tables
        vol = v.torus_volume(5, 100.0, 55.0, 22.0, v.VMaterial((0.8, 0.6, 0.2, 1.0), 0.8, 0.0))
        vol.material_id[vol.density <= 0] = 1
        vol.step_max = 0.0
    else:
        vol = copy.copy(shell(int(name)))
    return Case(vol.set_device_format(fmt), 1.0, 1)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["4", "5", "6", "sdf"])
def test_every_buffer_equals_the_reference_after_the_fill(renderer, name, fmt):
    case = volume_case(name, fmt)
    got = fill_and_check(renderer, case, f"volume {name}, format {fmt}")
    if name == "sdf":
        assert got["filled"] == 0
    elif fmt == _abi.FORMAT_F32:
        assert got["filled"] == {"4": 52, "5": 1136, "6": 11908}[name]
    else:
        assert got["filled"] > 0


@functools.lru_cache(maxsize=None)
def hand_made_case(name, fmt):
    d, wall, material, filled, lo, hi = F.hand_made_fields()[name]
    vol = v.VVoxelVolume(5, 100.0)
    vol.density, vol.material_id = d, F.hand_made_material(d)
    vol.step_max = 0.5 * vol.GetCellSize()  # both levels of the empty-space table live
    return Case(vol.set_device_format(fmt), wall, material), filled, lo, hi


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", sorted(F.hand_made_fields()))
def test_hand_made_fields(renderer, name, fmt):
    case, filled, lo, hi = hand_made_case(name, fmt)
    assert case.info["filled"] == filled and (not filled or (case.info["lo"], case.info["hi"]) == (lo, hi))  # the reference itself
    fill_and_check(renderer, case, f"{name}, format {fmt}")
    dense = buffers(renderer, EDITED)["dense"].view(np.uint32).reshape(case.stored.shape)
    walls = ~F.passable(F.decode(case.stored, fmt))
    assert np.array_equal(dense[walls], case.stored.view(np.uint32)[walls])  # walls — NaN, -0.0 and +0.0 among them — keep their bits
    if name == "channel":
        assert np.array_equal(dense[:, 5, :], case.stored.view(np.uint32)[:, 5, :])  # no part of the channel was taken for a cavity
    if name == "wall 0, ids untouched":
        assert np.array_equal(buffers(renderer, EDITED)["material"], case.material.reshape(-1))


def oracle_density(stored, fmt):
    """Floats that the oracle's own quantiser (format TEXEL16) turns into exactly the field +-q: (q + 0.5) * 0.01 with q's sign."""
    if fmt == _abi.FORMAT_F32:
        return np.array(stored, np.float32)
    mag = ((np.abs(stored) + np.float32(0.5)) * np.float32(0.01)).astype(np.float32)
    return np.where(np.signbit(stored), -mag, mag).astype(np.float32)


@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_after_the_fill(renderer, oracle_lib, fmt):
    sc = scenes.config3_voxelized(5, 16, device_format=fmt)
    vol = sc.volumes()[0]
    case = Case(vol, 1.0, 1)
    p = v.default_params(96, 54, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(p.width, p.height)
    renderer.params_override = p
    renderer.SetRendererMode(p.mode)
    renderer.Render()  # the scene's volume is resident in slot 0 now
    got = renderer.fill_enclosed(0, vol, 1.0, 1)
    check_result(got, case.info, "config3_voxelized(5)")
    assert got["filled"] > 1000 and vol.dirty_box is None and not vol.dirty  # the mirror follows without being dirtied
    assert_same_buffers(buffers(renderer, 0), case.device_bytes(), "filled slot against the reference")
    if fmt == _abi.FORMAT_F32:
        assert np.array_equal(vol.density.view(np.uint32), case.want_d.view(np.uint32)) and np.array_equal(vol.material_id, case.want_m)
    img = renderer.Render()
    t = renderer.last_timing()
    filled_vol = copy.copy(vol)
    filled_vol.density, filled_vol.material_id = oracle_density(case.want_d, fmt), np.array(case.want_m)
    ref_sc = copy.copy(sc)
    ref_sc.Objects = [copy.copy(o) for o in sc.Objects]
    ref_sc.Objects[0].Volume = filled_vol
    if fmt == _abi.FORMAT_TEXEL16:
        assert np.array_equal(R.texel16_field(filled_vol.density).view(np.uint32), case.want_d.view(np.uint32))
    want, st = OracleScene(ref_sc).render(p, threads=8)
    err = float(np.abs(img - want).max())
    print(f"format {fmt}: max |frame - oracle| {err:.3e}, hits {t['hits']}")
    assert err <= TOL
    assert {k: t[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS} and t["hits"] > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_fill_then_carve(renderer, fmt):
    """A SUBTRACT sphere that cuts into the tube of the filled torus (ring 8.6 cells out, tube 3.4 cells): the brush meets a solid."""
    case = volume_case("5", fmt)
    vol = case.vol
    upload_field(renderer, EDITED, vol, fmt, case.stored, case.material)
    renderer.fill_enclosed(EDITED, None, 1.0, 1)
    rec = v.sphere_brush(_abi.BRUSH_SUBTRACT, (24.6, 16.0, 16.0), 3.0, 0.0, 2.0, 0)
    got = renderer.apply_brushes(EDITED, None, [rec])
    stored, material = np.array(case.want_d), np.array(case.want_m)
    want = B.apply(stored, material, fmt, [rec], vol.VolumeExtends, vol.density_scale)
    assert got == want and got["written"] > 50
    assert_same_buffers(buffers(renderer, EDITED), case.device_bytes(stored, material), "carved after the fill")
    # every sample the fill wrote and the brush looked at is positive only where the brush's own -v is: no hollow behind the wall
    enclosed = case.want_d.view(np.uint32) != case.stored.view(np.uint32)
    s = B.brush_distance(rec, vol.N)
    looked = enclosed & (s < np.float32(rec.reach))
    positive = F.passable(B.decode(stored, fmt))
    assert int(looked.sum()) > 20 and int((looked & positive).sum()) > 5
    assert not (looked & positive & ~(-s > 0)).any()
    assert not (enclosed & ~looked & positive).any()


def test_refused_calls_change_nothing(renderer):
    case = volume_case("4", _abi.FORMAT_TEXEL16)
    upload_field(renderer, EDITED, case.vol, case.fmt, case.stored, case.material)
    before = buffers(renderer, EDITED)
    lib, ctx = renderer._lib, renderer._ctx
    res = _abi.vrt_fill_result()
    call = lambda ctx_, slot, wall, material: lib.vrt_volume_fill_enclosed(ctx_, slot, wall, material, C.byref(res))
    assert call(ctx, 7, 1.0, 1) == _abi.VRT_ERR_SLOT
    assert call(ctx, _abi.VRT_MAX_VOLUMES, 1.0, 1) == _abi.VRT_ERR_SLOT
    assert call(ctx, -1, 1.0, 1) == _abi.VRT_ERR_SLOT
    assert call(None, EDITED, 1.0, 1) == _abi.VRT_ERR_INVALID
    for wall in (float("nan"), float("inf"), float("-inf"), -1.0, -1e-30):
        assert call(ctx, EDITED, wall, 1) == _abi.VRT_ERR_INVALID, wall
    for material in (256, -2, 1 << 20):
        assert call(ctx, EDITED, 1.0, material) == _abi.VRT_ERR_INVALID, material
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")
    assert lib.vrt_volume_fill_enclosed(ctx, EDITED, 0.0, 255, None) == _abi.VRT_OK  # a wall of 0, id 255 and no result record are fine


def test_a_context_over_two_devices_fills_both(oracle_lib):
    results = {}
    for devices in ((0, 0), (0,)):
        vol = copy.copy(shell(5)).set_device_format(_abi.FORMAT_TEXEL16)
        vol.density, vol.material_id = np.array(vol.density), np.array(vol.material_id)
        with v.VHipRenderer(devices=devices) as r:
            r.upload_volume(EDITED, vol)
            res = r.fill_enclosed(EDITED, vol, 1.0, 1)
            results[devices] = (res, [buffers(r, EDITED, dev) for dev in range(len(devices))], vol.density.copy(), vol.material_id.copy())
    (res2, bufs2, d2, m2), (res1, bufs1, d1, m1) = results[(0, 0)], results[(0,)]
    assert res2 == res1 and res1["filled"] > 1000
    for dev in (0, 1):
        assert_same_buffers(bufs2[dev], bufs1[0], f"device {dev} of two against the single device")
    assert_same_buffers(bufs1[0], volume_case("5", _abi.FORMAT_TEXEL16).device_bytes(), "the single device against the reference")
    assert np.array_equal(d2.view(np.uint32), d1.view(np.uint32)) and np.array_equal(m2, m1)


def test_voxelizer_solid_on_the_device_writes_the_same_file(tmp_path):
    pos, nrm, idx = vx.torus_mesh(0.55, 0.22, 128, 64)
    cpos, cnrm, cidx = vx.cube_mesh(0.5)
    gltf = str(tmp_path / "scene.gltf")
    nodes = [{"name": "Torus", "mesh": 0}, {"name": "Cube", "mesh": 1, "translation": [0.0, 0.0, 2.0]}]
    vx.write_gltf(gltf, [("torus_5", pos, nrm, idx, None), ("cube_4", cpos, cnrm, cidx, None)], nodes)
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "voxelizer")
    outs = {}
    for name, extra in (("cpu", ["--solid"]), ("gpu", ["--gpu", "--solid"]), ("plain", [])):
        out = str(tmp_path / (name + ".vox"))
        r = subprocess.run([exe] + extra + ["--out", out, gltf], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "failed" not in r.stdout, r.stdout + r.stderr
        assert ("device voxelizer" in r.stdout) == (name == "gpu") and ("voxelizer, solid" in r.stdout) == (name != "plain")
        outs[name] = open(out, "rb").read()
    assert outs["cpu"] == outs["gpu"] and outs["cpu"] != outs["plain"]


def test_cpp_adaptor_fills_the_demo_model(tmp_path):
    """vrt_demo --solid: the red sphere built as a shell, filled through VHipRenderer::FillEnclosed, then carved on the device."""
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out = str(tmp_path / "solid.ppm")
    r = subprocess.run([exe, "--solid", "--frames", "4", "--size", "160x90", "--edit-brush", "12", "--edit-device", "--out", out],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("solid:")]
    assert line and int(line[0].split()[1]) > 5000 and "device brushes" in r.stdout
