"""vrt_volume_warp on the device: after the call the slot's dense grid, its material ids and the result record are those of the numpy
reference of the contract (tests/warp_ref.py), and every device buffer of the slot — bricks, cell records, both levels of the
empty-space table, the Cube table and the active box — is byte-identical to a full upload of the reference's result.  Tolerance 0
throughout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import volume_ref as R
import volumetricraytracer_amd as v
import warp_cases as K
import warp_ref as W
from volumetricraytracer_amd import _abi
from test_volume_fill_gpu import EDITED, FULL, assert_same_buffers, buffers, upload_field
from test_volume_warp import accepted_records, good_record, refused_records

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_slots(request):
    """Tests here upload into the session renderer's slots behind SyncWithScene's back: the slots start unused and are freed after."""
    def free():
        if "renderer" in request.fixturenames:
            r = request.getfixturevalue("renderer")
            for slot in (EDITED, FULL):
                r._uploaded.pop(slot, None)
                r._lib.vrt_volume_free(r._ctx, slot)  # VRT_ERR_SLOT when unused
    free()
    yield
    free()


def check_result(got, want, what):
    assert got["written"] == want["written"], (what, got, want)
    if want["written"]:
        assert got == want, (what, got, want)
    else:
        assert all(l > h for l, h in zip(got["lo"], got["hi"])), (what, got)


def warp_and_check(r, what, stored, material, fmt, rec, want, table):
    """The field uploaded, one call, then the slot against the reference and against a full upload of the reference's result.  Returns
    (the buffers before the call, the buffers after it)."""
    N = stored.shape[0]
    what = f"{what} ({N}^3, format {fmt}, tables {table})"
    vol = K.volume(N, table)
    upload_field(r, EDITED, vol, fmt, stored, material)
    before = buffers(r, EDITED)
    want_d, want_m, info = want[:3]
    got = r.warp_volume(EDITED, rec)
    check_result(got, info, what)
    have = buffers(r, EDITED)
    assert np.array_equal(have["dense"].view(np.uint32), want_d.view(np.uint32).reshape(-1)), what
    assert np.array_equal(have["material"], want_m.reshape(-1)), what
    upload_field(r, FULL, vol, fmt, want_d, want_m)
    full = buffers(r, FULL)
    if not table:
        full["active_box"] = None  # a slot without the tables keeps whatever box it had before: not a buffer of this volume
    assert_same_buffers(have, full, what + " against a full upload")
    if info["written"] == 0:
        assert_same_buffers(have, before, what + ": nothing written, nothing changed")
    return before, have


@pytest.mark.parametrize("fmt", K.FORMATS)
@pytest.mark.parametrize("N", K.SIZES)
def test_device_warp_equals_the_reference_over_the_sweep(renderer, N, fmt):
    stored, material = K.field(N, fmt)
    for what, rec in K.sweep(N):
        want = K.sweep_reference(N, fmt, rec)
        assert want[2]["written"] > 0, what
        for table in (True, False):
            warp_and_check(renderer, what, stored, material, fmt, rec, want, table)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_every_read_sees_the_volume_before_the_call(renderer, fmt):
    """The 65^3 case that tells the rule from an in-place pass (tests/test_volume_warp.py, test_jacobi_matters): the box starts on samples
    that are multiples of neither 4 nor 8, spans several workgroups and bricks per axis, and sources lie in other bricks than their
    destinations."""
    stored, material, rec = K.jacobi_case(fmt)
    want = K.reference(stored, material, fmt, rec, "jacobi")
    info = want[2]
    assert all(h - l + 1 >= 38 for l, h in zip(info["lo"], info["hi"])) and all(l % 4 != 0 and l > 8 for l in info["lo"]), info
    warp_and_check(renderer, "a ball of 40 cells grabbed", stored, material, fmt, rec, want, table=True)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_a_source_beyond_the_grid_is_the_face(renderer, fmt):
    stored, material, rec = K.clamp_case(fmt)
    want = K.reference(stored, material, fmt, rec, "clamp")
    assert want[2]["written"] > 100 and want[2]["lo"][2] == 0
    warp_and_check(renderer, "clamped at z = 0", stored, material, fmt, rec, want, table=False)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_an_identity_motion_and_a_region_outside_the_grid_change_nothing(renderer, fmt):
    N = 17
    stored, material = K.field(N, fmt)
    outside = v.warp_record(_abi.BRUSH_CAPSULE, (-30.0, 8.0, 8.0), (-12.0, 8.0, 8.0), 4.0, pull=K.grab((1.0, 2.0, 3.0)), material=5)
    for what, rec in [(f"identity, material {r.material}", r) for r in K.identity_cases(N)] + [("wholly outside", outside)]:
        want = W.warp(stored, material, fmt, rec)
        assert want[2]["written"] == 0
        warp_and_check(renderer, what, stored, material, fmt, rec, want, table=True)  # compares with the buffers before the call


def test_material_only_writes_rebuild_nothing(renderer):
    stored, material, rec = K.material_only_case()
    want = K.reference(stored, material, R.F32, rec, "material only")
    assert want[3] == 0 and want[2]["written"] > 100
    before, have = warp_and_check(renderer, "material only", stored, material, R.F32, rec, want, table=True)
    before["material"] = have["material"]  # checked against the reference above; every other buffer is as it was
    assert_same_buffers(have, before, "material only: no density changed, nothing rebuilt")


@pytest.mark.parametrize("fmt", K.FORMATS)
@pytest.mark.parametrize("N", K.SMALL)
def test_device_warp_on_the_smallest_grids(renderer, N, fmt):
    """Grids of 2, 3 and 5 samples: the cell clamp to N - 2 and one brick are the whole story."""
    stored, material = K.small_field(N, fmt)
    written = 0
    for what, rec in K.small_cases(N):
        want = K.reference(stored, material, fmt, rec, ("small", N))
        warp_and_check(renderer, what, stored, material, fmt, rec, want, table=True)
        written += want[2]["written"]
    assert written > 0


def test_the_host_mirror_follows(renderer):
    N = 17
    stored, material = K.field(N, R.F32)
    vol = K.volume(N, True)
    vol.density, vol.material_id = np.array(stored), np.array(material)
    renderer.upload_volume(EDITED, vol)
    what, rec = K.sweep(N)[2]
    want_d, want_m, info, _ = K.sweep_reference(N, R.F32, rec)
    vol.dirty = False
    got = renderer.warp_volume(EDITED, rec, vol)
    assert got == info and info["written"] > 0 and not vol.dirty
    assert np.array_equal(vol.density.view(np.uint32), want_d.view(np.uint32)) and np.array_equal(vol.material_id, want_m)


def test_refused_calls_change_nothing(renderer):
    N = 17
    stored, material = K.field(N, R.TEXEL16)
    upload_field(renderer, EDITED, K.volume(N, True), R.TEXEL16, stored, material)
    before = buffers(renderer, EDITED)
    lib, ctx = renderer._lib, renderer._ctx
    res = _abi.vrt_brush_result()
    good = good_record()
    call = lambda slot, rec: lib.vrt_volume_warp(ctx, slot, rec, C.byref(res))
    assert lib.vrt_volume_warp(None, EDITED, C.byref(good), C.byref(res)) == _abi.VRT_ERR_INVALID
    assert call(EDITED, None) == _abi.VRT_ERR_INVALID
    for slot in (7, -1, _abi.VRT_MAX_VOLUMES):
        assert call(slot, C.byref(good)) == _abi.VRT_ERR_SLOT, slot
    for what, rec in refused_records():
        assert call(EDITED, C.byref(rec)) == _abi.VRT_ERR_INVALID, what
        assert call(7, C.byref(rec)) == _abi.VRT_ERR_INVALID, what  # the record is judged before the slot
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")
    for what, rec in accepted_records():
        assert call(EDITED, C.byref(rec)) == _abi.VRT_OK, what
    assert lib.vrt_volume_warp(ctx, EDITED, C.byref(good), None) == _abi.VRT_OK  # no result record is fine


def test_cpp_adaptor_grabs_the_demo_model(tmp_path):
    """vrt_demo --edit-grab: every frame a ball around the brush position of the filled red sphere is pulled outwards through
    VHipRenderer::WarpVolume, before the written box is redistanced; the flag without --edit-device is refused."""
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out = str(tmp_path / "grabbed.ppm")
    common = [exe, "--solid", "--frames", "4", "--size", "160x90", "--out", out]
    r = subprocess.run(common + ["--edit-brush", "6", "--edit-device", "--edit-grab", "1.5", "--sdf", "3"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("grab:")]
    assert line and float(line[0].split()[1]) == 1.5 and int(line[0].split()[4]) > 1000, r.stdout
    assert "device grabs" in r.stdout
    r = subprocess.run(common + ["--edit-brush", "6", "--edit-grab", "1.5"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 1 and "--edit-grab" in r.stderr
