"""CSG sculpt brushes on the device (vrt_volume_apply_brushes) and the box read-back (vrt_volume_download_region): after every
call each device buffer of the slot — dense grid, materials, bricks, cell records, both levels of the empty-space table, the Cube
table and the active box — is byte-identical to the numpy reference of the brush arithmetic (tests/brush_ref.py) pushed through the
reference of the upload (tests/volume_ref.py), and to a full upload of that field; so frames and counters are those of the existing
contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brush_ref as B
import volume_ref as R
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
EDITED, FULL = 0, 1  # slots: the brushed volume, and a full upload of the reference's field
FORMATS = [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16]
ADD, SUB, PAINT = _abi.BRUSH_ADD, _abi.BRUSH_SUBTRACT, _abi.BRUSH_PAINT


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


def make_volume(kind, res, fmt):
    vol = v.torus_volume(res, 100.0, 55.0, 22.0, v.VMaterial((0.8, 0.6, 0.2, 1.0), 0.8, 0.0))
    vol.material_id[vol.density <= 0] = 1
    if kind == "shell":  # both levels of the empty-space table live
        vol.step_max = 0.5 * vol.GetCellSize()
    return vol.set_device_format(fmt)


class Reference:
    """The reference's own copy of what the device stores for `vol`: the DENSE field (F32: the floats; TEXEL16: +-q) and the
    material ids, edited by brush_ref."""

    def __init__(self, vol):
        self.vol, self.fmt = vol, int(vol.device_format)
        self.stored = R.dense_field(np.array(vol.density, np.float32), self.fmt)
        self.material = np.array(vol.material_id, np.uint8)

    def apply(self, recs):
        return B.apply(self.stored, self.material, self.fmt, recs, self.vol.VolumeExtends, self.vol.density_scale)

    def device_bytes(self):
        return R.device_bytes(self.stored, self.material, self.fmt, self.vol.density_scale, self.vol.step_max)

    def upload(self, r, slot):
        """A full upload of exactly this field: the floats (F32), or the RGBA8 texels of +-q (TEXEL16 — uploading q * 0.01 as
        floats would quantise a second time)."""
        lib, ctx, vol = r._lib, r._ctx, self.vol
        if self.fmt == _abi.FORMAT_F32:
            _abi.check(lib.vrt_set_volume_format(ctx, _abi.FORMAT_F32), "vrt_set_volume_format")
            d, m = np.ascontiguousarray(self.stored), np.ascontiguousarray(self.material)
            rc = lib.vrt_volume_upload(ctx, slot, vol.Resolution, vol.VolumeExtends, d.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p))
        else:
            tex = B.texels_of(self.stored, self.material)
            rc = lib.vrt_volume_upload_texels(ctx, slot, vol.Resolution, vol.VolumeExtends, tex.ctypes.data_as(C.c_void_p))
        _abi.check(rc, "vrt_volume_upload*")
        _abi.check(lib.vrt_volume_set_metric(ctx, slot, float(vol.density_scale), float(vol.step_max)), "vrt_volume_set_metric")


def check_result(got, want, what):
    assert got["written"] == want["written"], (what, got, want)
    if want["written"] == 0:
        assert all(l > h for l, h in zip(got["lo"], got["hi"])), (what, got)
    else:
        assert got["lo"] == want["lo"] and got["hi"] == want["hi"], (what, got, want)


def apply_and_check(r, ref, recs, what, full=True):
    """One call on slot EDITED and on the reference; every buffer against both witnesses."""
    got = r.apply_brushes(EDITED, None, recs)
    want = ref.apply(recs)
    print(f"{what}: {len(recs)} records, written {got['written']} (reference {want['written']}), box {got['lo']}..{got['hi']}")
    check_result(got, want, what)
    have = buffers(r, EDITED)
    assert_same_buffers(have, ref.device_bytes(), what + " against the reference")
    if full:
        ref.upload(r, FULL)
        assert_same_buffers(have, buffers(r, FULL), what + " against a full upload")
    return got


def random_record(rng, n, reach_max=6.0):
    """Any shape and op, hard or blended, fractional positions, centres up to a few cells outside the grid."""
    shape = int(rng.integers(0, 3))
    op = int(rng.choice([ADD, SUB, SUB, ADD, PAINT]))
    a = [float(x) for x in rng.uniform(-2.0, n + 1.0, 3)]
    blend = float(rng.choice([0.0, rng.uniform(0.5, 3.0)]))
    reach = float(rng.uniform(1.0, reach_max))
    material = int(rng.integers(0, 256)) if op == PAINT else int(rng.choice([-1, 0, int(rng.integers(1, 256))]))
    size = float(rng.uniform(1.0, max(1.5, n / 6)))
    if shape == _abi.BRUSH_SPHERE:
        return v.sphere_brush(op, a, size, blend, reach, material)
    if shape == _abi.BRUSH_BOX:
        half = [float(x) for x in rng.uniform(0.5, max(1.0, n / 6), 3)]
        return v.box_brush(op, a, half, float(rng.choice([0.0, rng.uniform(0.0, 2.0)])), blend, reach, material)
    b = [x + float(d) for x, d in zip(a, rng.uniform(-n / 4, n / 4, 3))]
    b[0] += 0.25  # never a == b
    return v.capsule_brush(op, a, b, min(size, 4.0), blend, reach, material)


def call_sequence(vol, rng):
    """(what, records) per call: every shape and op, hard and blended, fractional centres, brushes half outside each face, one wholly
    outside, footprints covering the whole grid, a call with 32 records, PAINT over solid and over empty space."""
    n = vol.N
    s = (n - 1) / 64.0  # positions below are written for N = 65
    P = lambda *p: tuple(x * s for x in p)
    big = max(1.0, 5.0 * s)
    calls = [
        ("hard subtract sphere", [v.sphere_brush(SUB, P(50, 32, 40), big, 0.0, 2.0, 0)]),
        ("blended add sphere, fractional centre", [v.sphere_brush(ADD, P(32.4, 50.3, 39.7), max(1.0, 4.0 * s), 2.0, 6.0, 2)]),
        ("hard add box", [v.box_brush(ADD, P(14, 32, 30), (max(0.5, 4 * s), max(0.5, 3 * s), max(0.5, 6 * s)), 0.0, 0.0, 5.0, 3)]),
        ("blended subtract rounded box", [v.box_brush(SUB, P(15.5, 33, 31.25), (max(0.5, 3 * s), max(0.5, 5 * s), max(0.5, 3 * s)), 1.0, 1.5, 2.0, -1)]),
        ("hard add capsule", [v.capsule_brush(ADD, P(20, 20, 30), P(44, 26, 34), max(0.75, 2.5 * s), 0.0, 4.0, 4)]),
        ("blended subtract capsule", [v.capsule_brush(SUB, P(24, 30, 28), P(40.5, 34, 36), max(0.75, 3.0 * s), 1.5, 2.0, 0)]),
    ]
    for axis in range(3):  # half outside face 0 and face N-1 of every axis
        for k, at in enumerate((0.0, float(n - 1))):
            c = [float(x) for x in rng.uniform(0.25 * n, 0.75 * n, 3)]
            c[axis] = at + (0.3 if k == 0 else -0.3)
            op = ADD if (axis + k) % 2 == 0 else SUB
            calls.append((f"half outside axis {axis} at {at}", [v.sphere_brush(op, c, max(1.0, n / 8), float(k), 3.0, 6 + axis)]))
    calls.append(("paint over empty space", [v.sphere_brush(PAINT, P(4, 4, 4), max(0.5, 2.0 * s), material=77)]))
    calls.append(("wholly outside", [v.sphere_brush(ADD, (-20.0, n / 2, n / 2), 4.0, 1.0, 3.0, 1),
                                     v.box_brush(SUB, (n / 2, n + 30.0, n / 2), (3, 3, 3), 0.0, 0.0, 2.0, 0)]))
    calls.append(("add with a footprint over the whole grid", [v.sphere_brush(ADD, P(32.5, 31.2, 33), max(1.0, 3.0 * s), 1.0, 4.0 * n, 7)]))
    calls.append(("32 records", [random_record(rng, n) for _ in range(_abi.MAX_BRUSHES)]))
    calls.append(("paint over solid", [v.box_brush(PAINT, P(32, 32, 32), (n, max(0.5, 8 * s), n), material=200)]))
    for i in range(3):
        calls.append((f"random {i}", [random_record(rng, n) for _ in range(int(rng.integers(1, 6)))]))
    calls.append(("subtract box over the whole grid", [v.box_brush(SUB, P(32, 32, 32), (1.5 * n,) * 3, 0.0, 0.0, 2.0, 0)]))
    calls.append(("add into the emptied volume", [v.sphere_brush(ADD, P(20, 40, 30), max(1.0, 6.0 * s), 0.0, 4.0 * n, 9),
                                                  v.capsule_brush(ADD, P(10, 10, 10), P(50, 50, 50), max(0.75, 2.0 * s), 2.0, 8.0, 11)]))
    return calls


def run_sequence(r, vol, rng):
    for slot in (EDITED, FULL):
        r._lib.vrt_volume_free(r._ctx, slot)
    r.upload_volume(EDITED, vol)
    ref = Reference(vol)
    assert_same_buffers(buffers(r, EDITED), ref.device_bytes(), "before any brush")
    out = {}
    for what, recs in call_sequence(vol, rng):
        out[what] = apply_and_check(r, ref, recs, what)
    return out, ref


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", ["torus", "shell"])
def test_every_buffer_equals_the_reference_after_each_call(renderer, fmt, kind):
    rng = np.random.default_rng(23 + fmt + 2 * (kind == "shell"))
    vol = make_volume(kind, 6, fmt)
    got, ref = run_sequence(renderer, vol, rng)
    n = vol.N
    assert got["hard subtract sphere"]["written"] > 100 and got["32 records"]["written"] > 100
    assert got["wholly outside"]["written"] == 0
    assert got["paint over solid"]["written"] > 0 and got["paint over empty space"]["written"] == 0
    whole = got["subtract box over the whole grid"]
    assert whole["lo"] == (0, 0, 0) and whole["hi"] == (n - 1,) * 3 and (ref.material <= 11).all()
    assert renderer.apply_brushes(EDITED, None, []) == {"written": 0, "lo": (n, n, n), "hi": (-1, -1, -1)}  # n == 0: OK, nothing changes
    assert_same_buffers(buffers(renderer, EDITED), ref.device_bytes(), "after an empty call")


def test_untouched_texels_keep_their_bits(renderer):
    """A hard SUBTRACT sphere in empty space with a large reach: -v stays below the field everywhere, so no sample is written — while
    10068 texels of its footprint would change under decode + encode."""
    vol = make_volume("shell", 6, _abi.FORMAT_TEXEL16)
    rec = v.sphere_brush(SUB, (32, 32, 32), 2.0, 0.0, 20.0, 0)
    ref = Reference(vol)
    before = ref.stored.copy()
    foot = B.brush_distance(rec, vol.N) < np.float32(20.0)
    assert int((foot & (R.texel16_field(B.decode(before, R.TEXEL16)) != before)).sum()) == 10068
    assert ref.apply([rec])["written"] == 0 and np.array_equal(ref.stored.view(np.uint32), before.view(np.uint32))
    renderer.upload_volume(EDITED, vol)
    have = buffers(renderer, EDITED)
    got = renderer.apply_brushes(EDITED, None, [rec])
    assert got["written"] == 0 and all(l > h for l, h in zip(got["lo"], got["hi"]))
    assert_same_buffers(buffers(renderer, EDITED), have, "a brush that writes nothing")
    assert_same_buffers(have, ref.device_bytes(), "against the reference")


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_call_equals_n_calls(renderer, fmt):
    rng = np.random.default_rng(5)
    vol = make_volume("shell", 6, fmt)
    recs = [v.sphere_brush(SUB, (50, 32, 40), 5.0, 0.0, 2.0, 0), v.sphere_brush(ADD, (32.4, 50.3, 39.7), 4.0, 2.0, 6.0, 2),
            v.capsule_brush(SUB, (24, 30, 28), (40.5, 34, 36), 3.0, 1.5, 2.0, 0), v.box_brush(ADD, (48, 30, 38), (4, 3, 5), 1.0, 1.0, 4.0, 5),
            v.sphere_brush(PAINT, (48, 30, 38), 7.0, material=8)] + [random_record(rng, vol.N) for _ in range(3)]
    renderer.upload_volume(EDITED, vol)
    one = renderer.apply_brushes(EDITED, None, recs)
    renderer.upload_volume(FULL, vol)
    for rec in recs:
        renderer.apply_brushes(FULL, None, [rec])
    assert one["written"] > 1000
    assert_same_buffers(buffers(renderer, EDITED), buffers(renderer, FULL), "8 records in one call against 8 calls")
    ref = Reference(vol)
    check_result(one, ref.apply(recs), "8 records")
    assert_same_buffers(buffers(renderer, EDITED), ref.device_bytes(), "8 records against the reference")


@pytest.mark.parametrize("res", [0, 1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
def test_small_resolutions(renderer, res, fmt):
    rng = np.random.default_rng(300 + res)
    for kind in ("torus", "shell"):
        run_sequence(renderer, make_volume(kind, res, fmt), rng)


def edited_scene(fmt):
    sc = scenes.config3_torus(6, 16)
    vol = sc.volumes()[0].set_device_format(fmt)
    vol.step_max = 0.5 * vol.GetCellSize()
    return sc, vol


def carve_records():
    """The side of the torus (ring around z, 17.6 cells out, tube 7 cells) that faces the camera: two bites, one lump."""
    return [v.sphere_brush(SUB, (50, 32, 40), 5.0, 0.0, 2.0, 0), v.sphere_brush(SUB, (57, 32, 32), 4.0, 1.0, 2.0, 0),
            v.sphere_brush(ADD, (32, 50, 40), 4.0, 0.0, 2.0, 1)]


def frame_cases(fmt):
    paths = (_abi.PATH_DENSE, _abi.PATH_BRICK, _abi.PATH_AUTO) + ((_abi.PATH_CELLS,) if fmt == _abi.FORMAT_TEXEL16 else ())
    cases = [(path, mode, False) for mode in (_abi.MODE_INTERP_NOTEX, _abi.MODE_CUBE_NOTEX) for path in paths]
    return cases + [(_abi.PATH_AUTO, _abi.MODE_INTERP_NOTEX, True)]


def render_case(r, cell, case):
    path, mode, shadow = case
    p = v.default_params(256, 144, cell, 255, shadow=shadow, mode=mode, path=path)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(mode)
    img = r.Render()
    t = r.last_timing()
    return p, img, {k: t[k] for k in STAT_KEYS}


@pytest.mark.parametrize("fmt", FORMATS)
def test_frames_after_brushes(oracle_lib, fmt):
    sc, vol = edited_scene(fmt)
    cell = scenes.min_cell(sc)
    cases = frame_cases(fmt)
    ref = Reference(vol)
    with v.VHipRenderer() as r:
        r.SetSceneToRender(sc)
        _, before, _ = render_case(r, cell, cases[0])
        got = r.apply_brushes(0, vol, carve_records())
        check_result(got, ref.apply(carve_records()), "carve")
        assert got["written"] > 500 and vol.dirty_box is None and not vol.dirty  # the mirror follows without being dirtied
        assert_same_buffers(buffers(r, 0), ref.device_bytes(), "carved slot against the reference")
        # the mirror holds the device's (decoded) values in the written box; outside it a TEXEL16 mirror keeps the caller's floats
        (x0, y0, z0), (x1, y1, z1) = got["lo"], got["hi"]
        box = (slice(x0, x1 + 1), slice(z0, z1 + 1), slice(y0, y1 + 1)) if fmt == _abi.FORMAT_TEXEL16 else (slice(None),) * 3
        assert np.array_equal(vol.density[box].view(np.uint32), B.decode(ref.stored, ref.fmt)[box].view(np.uint32))
        assert np.array_equal(vol.material_id, ref.material)
        edited = []
        for case in cases:
            p, img, stats = render_case(r, cell, case)
            assert stats["hits"] > 0
            if fmt == _abi.FORMAT_F32:  # the oracle marches the host mirror apply_brushes maintained
                want, st = OracleScene(sc).render(p, threads=8)
                err = float(np.abs(img - want).max())
                print(f"case {case}: max |frame - oracle| {err:.3e}")
                assert err <= TOL, case
                assert stats == {k: st[k] for k in STAT_KEYS}, case
            edited.append((img, stats))
        assert not np.array_equal(edited[0][0], before)
        if fmt == _abi.FORMAT_F32:
            vol.dirty = True  # the mirror uploaded whole
        else:  # the mirror holds decoded values, which would quantise a second time: upload the reference's texel field instead
            tex = B.texels_of(ref.stored, ref.material)
            _abi.check(r._lib.vrt_volume_upload_texels(r._ctx, 0, vol.Resolution, vol.VolumeExtends, tex.ctypes.data_as(C.c_void_p)),
                       "vrt_volume_upload_texels")
        for case, (img, stats) in zip(cases, edited):
            _, again, stats2 = render_case(r, cell, case)
            assert np.array_equal(again, img) and stats2 == stats, case


@pytest.mark.parametrize("fmt", FORMATS)
def test_download_region_equals_the_slice_of_a_full_download(renderer, fmt):
    rng = np.random.default_rng(41 + fmt)
    vol = make_volume("shell", 5, fmt)
    vol.material_id = ((np.arange(vol.N ** 3) * 7 + 3) % 256).astype(np.uint8).reshape((vol.N,) * 3)
    renderer.upload_volume(EDITED, vol)
    renderer.apply_brushes(EDITED, None, [v.sphere_brush(SUB, (20, 16, 16), 5.0, 1.0, 2.0, -1)])
    n = vol.N
    whole = renderer.download_volume(EDITED, vol.Resolution, vol.VolumeExtends)
    boxes = [((0, 0, 0), (n - 1,) * 3), ((n - 1,) * 3, (n - 1,) * 3), ((0, 0, 0), (0, 0, 0))]
    for _ in range(12):
        lo = rng.integers(0, n, 3)
        hi = [int(rng.integers(l, n)) for l in lo]
        boxes.append((tuple(int(x) for x in lo), tuple(hi)))
    before = buffers(renderer, EDITED)
    for lo, hi in boxes:
        d, m = renderer.download_region(EDITED, lo, hi)
        box = (slice(lo[0], hi[0] + 1), slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1))
        assert np.array_equal(d.view(np.uint32), whole.density[box].view(np.uint32)), (lo, hi)
        assert np.array_equal(m, whole.material_id[box]), (lo, hi)
        if fmt == _abi.FORMAT_F32:  # what came down goes up again unchanged
            rec = np.zeros(d.shape, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
            rec["material"], rec["density"] = m, d
            size = (C.c_int * 3)(*(h - l + 1 for l, h in zip(lo, hi)))
            _abi.check(renderer._lib.vrt_volume_update_voxels(renderer._ctx, EDITED, (C.c_int * 3)(*lo), size,
                                                              np.ascontiguousarray(rec).ctypes.data_as(C.c_void_p)), "vrt_volume_update_voxels")
            assert_same_buffers(buffers(renderer, EDITED), before, f"update_voxels(download_region({lo}, {hi}))")
    lib, ctx = renderer._lib, renderer._ctx
    out = np.zeros(8 * n ** 3, np.uint8).ctypes.data_as(C.c_void_p)
    box = lambda *a: (C.c_int * 3)(*a)
    assert lib.vrt_volume_download_region(ctx, 7, box(0, 0, 0), box(1, 1, 1), out) == _abi.VRT_ERR_SLOT
    for o, s in (((0, 0, 0), (n + 1, 1, 1)), ((n - 1, 0, 0), (2, 1, 1)), ((0, -1, 0), (1, 1, 1)), ((0, 0, n), (1, 1, 1)), ((0, 0, 0), (0, 1, 1))):
        assert lib.vrt_volume_download_region(ctx, EDITED, box(*o), box(*s), out) == _abi.VRT_ERR_INVALID, (o, s)
    assert lib.vrt_volume_download_region(ctx, EDITED, box(0, 0, 0), box(1, 1, 1), None) == _abi.VRT_ERR_INVALID


def test_a_context_over_two_devices_brushes_both(oracle_lib):
    results = {}
    for devices in ((0, 0), (0,)):
        vol = make_volume("shell", 6, _abi.FORMAT_TEXEL16)
        with v.VHipRenderer(devices=devices) as r:
            r.upload_volume(EDITED, vol)
            res = r.apply_brushes(EDITED, vol, carve_records() + [v.sphere_brush(PAINT, (32, 50, 40), 5.0, material=6)])
            results[devices] = (res, [buffers(r, EDITED, dev) for dev in range(len(devices))], vol.density.copy(), vol.material_id.copy())
    (res2, bufs2, d2, m2), (res1, bufs1, d1, m1) = results[(0, 0)], results[(0,)]
    assert res2 == res1 and res1["written"] > 500
    for dev in (0, 1):
        assert_same_buffers(bufs2[dev], bufs1[0], f"device {dev} of two against the single device")
    assert np.array_equal(d2.view(np.uint32), d1.view(np.uint32)) and np.array_equal(m2, m1)


def test_refused_calls_change_nothing(renderer):
    vol = make_volume("shell", 5, _abi.FORMAT_TEXEL16)
    renderer.upload_volume(EDITED, vol)
    before = buffers(renderer, EDITED)
    lib, ctx = renderer._lib, renderer._ctx
    good = lambda: v.sphere_brush(SUB, (16, 16, 16), 5.0, 1.0, 2.0, 0)
    res = _abi.vrt_brush_result()

    def call(slot, n, recs):
        arr = (_abi.vrt_brush * max(1, len(recs)))(*recs) if recs is not None else None
        return lib.vrt_volume_apply_brushes(ctx, slot, n, arr, C.byref(res))

    assert call(7, 1, [good()]) == _abi.VRT_ERR_SLOT
    assert call(_abi.VRT_MAX_VOLUMES, 1, [good()]) == _abi.VRT_ERR_SLOT
    assert call(EDITED, 1, None) == _abi.VRT_ERR_INVALID
    assert call(EDITED, -1, [good()]) == _abi.VRT_ERR_INVALID
    assert call(EDITED, _abi.MAX_BRUSHES + 1, [good()] * (_abi.MAX_BRUSHES + 1)) == _abi.VRT_ERR_INVALID

    def bad(**fields):
        rec = fields.pop("base", None) or good()
        for k, val in fields.items():
            if isinstance(val, tuple):
                for i, x in enumerate(val):
                    getattr(rec, k)[i] = x
            else:
                setattr(rec, k, val)
        return rec

    box = lambda: v.box_brush(ADD, (16, 16, 16), (3, 3, 3), 1.0, 0.0, 2.0, 1)
    cap = lambda: v.capsule_brush(ADD, (10, 16, 16), (20, 16, 16), 2.0, 0.0, 2.0, 1)
    inf, nan = float("inf"), float("nan")
    cases = {
        "unknown shape": bad(shape=3), "negative shape": bad(shape=-1), "unknown op": bad(op=3), "negative op": bad(op=-1),
        "nan centre": bad(a=(nan, 16.0, 16.0)), "inf centre": bad(a=(16.0, inf, 16.0)), "nan b of a sphere": bad(b=(0.0, 0.0, nan)),
        "inf radius": bad(radius=inf), "nan blend": bad(blend=nan), "inf reach": bad(reach=inf), "nan reach": bad(reach=nan),
        "zero radius": bad(radius=0.0), "negative radius": bad(radius=-1.0), "zero capsule radius": bad(base=cap(), radius=0.0),
        "zero half size": bad(base=box(), b=(3.0, 0.0, 3.0)), "negative half size": bad(base=box(), b=(-3.0, 3.0, 3.0)),
        "zero reach": bad(reach=0.0), "negative reach": bad(reach=-2.0), "negative blend": bad(blend=-0.5),
        "negative rounding": bad(base=box(), radius=-0.25), "capsule a == b": bad(base=cap(), b=(10.0, 16.0, 16.0)),
        "material 256": bad(material=256), "material -2": bad(material=-2), "paint without a material": bad(op=PAINT, material=-1),
        "reserved word 0": bad(reserved_=(1, 0, 0, 0)), "reserved word 3": bad(reserved_=(0, 0, 0, 5)),
    }
    for what, rec in cases.items():
        assert call(EDITED, 1, [rec]) == _abi.VRT_ERR_INVALID, what
        assert call(EDITED, 3, [good(), good(), rec]) == _abi.VRT_ERR_INVALID, what + " (after two good records)"
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")
    assert call(EDITED, 0, None) == _abi.VRT_OK and call(EDITED, 0, [good()]) == _abi.VRT_OK  # n == 0 changes nothing
    assert_same_buffers(buffers(renderer, EDITED), before, "after empty calls")
    assert call(EDITED, 1, [box()]) == _abi.VRT_OK and res.written > 0  # a rounding of 0 and a blend of 0 are fine
    assert call(EDITED, 1, [bad(base=box(), radius=0.0)]) == _abi.VRT_OK


def _frame_renderer(r, sc, p):
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)


def test_a_frame_begun_before_a_brush_renders_the_old_volume(oracle_lib):
    sc, vol = edited_scene(_abi.FORMAT_F32)
    p = v.default_params(256, 144, scenes.min_cell(sc), 255, shadow=True)
    with v.VHipRenderer() as r:
        _frame_renderer(r, sc, p)
        before = r.Render()
        r.render_begin(0, p)
        r.apply_brushes(0, vol, carve_records())  # waits for the frame on slot 0
        r.render_begin(1, p)
        first, second = r.render_end(0, p), r.render_end(1, p)
        after = r.Render()
    assert np.array_equal(first, before)
    assert np.array_equal(second, after)
    assert not np.array_equal(before, after)


def test_a_captured_frame_replays_over_the_brushed_volume(renderer, oracle_lib):
    """Device pointers survive a brush call: a render_rows launch captured before it replays the brushed volume."""
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
    renderer.apply_brushes(0, vol, carve_records())
    assert vol.dirty_box is None and not vol.dirty
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


def test_cpp_adaptor_device_brushes_change_the_frame(tmp_path):
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    outs = {}
    for name, extra in (("device", ["--edit-brush", "6", "--edit-device"]), ("plain", [])):
        out = str(tmp_path / (name + ".ppm"))
        r = subprocess.run([exe, "--frames", "10", "--size", "320x180", "--out", out] + extra, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr
        outs[name] = open(out, "rb").read()
        if name == "device":
            assert "device brushes" in r.stdout
    assert outs["device"] != outs["plain"]  # the brushes changed the frame
