"""vrt_volume_smooth on the device: after the call the slot's dense grid, its material ids and the result record are those of the
numpy reference of the contract (tests/smooth_ref.py), and every device buffer of the slot — bricks, cell records, both levels of the
empty-space table, the Cube table and the active box — is byte-identical to a full upload of the reference's result.  Tolerance 0
throughout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import smooth_cases as K
import smooth_ref as S
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from test_volume_fill_gpu import EDITED, FULL, assert_same_buffers, buffers, upload_field
from test_volume_smooth import accepted_records, good_record, refused_records

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


def smooth_and_check(r, what, stored, material, fmt, rec, want, table):
    """The field uploaded, one call, then the slot against the reference and against a full upload of the reference's result."""
    N = stored.shape[0]
    what = f"{what} ({N}^3, format {fmt}, tables {table})"
    vol = K.volume(N, table)
    upload_field(r, EDITED, vol, fmt, stored, material)
    before = buffers(r, EDITED)
    want_d, want_m, info = want
    got = r.smooth_volume(EDITED, rec)
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
    return info


@pytest.mark.parametrize("fmt", K.FORMATS)
@pytest.mark.parametrize("N", K.SIZES)
def test_device_smooth_equals_the_reference_over_the_sweep(renderer, N, fmt):
    stored, material = K.field(N, fmt)
    for what, rec in K.sweep(N):
        for table in (True, False):
            info = smooth_and_check(renderer, what, stored, material, fmt, rec, K.sweep_reference(N, fmt, rec), table)
            assert info["written"] > 0, what


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_a_region_of_several_workgroups_bricks_and_tiles_per_axis(renderer, fmt):
    """65^3, a ball of 40 cells across about (34.5, 29.4, 34.9): its box starts on samples that are no multiple of 8 (nor of 4, the
    bricks), spans six tiles of a pass per axis and is far from every face, so every tile has its full halo of neighbours from other
    tiles.  Three iterations with a rebound: six passes, ending in the first copy."""
    N = 65
    stored = R.dense_field(S.noisy_sphere(N, K.sphere_radius(N), 0.3, seed=N), fmt)
    material = (stored <= 0).astype(np.uint8)
    rec = v.smooth_record(_abi.BRUSH_SPHERE, (34.5, 29.4, 34.9), (0, 0, 0), 20.0, strength=0.5, iterations=3, falloff=3.0, rebound=0.5, material=4)
    want = S.smooth(stored, material, fmt, rec)
    info = want[2]
    spans = [h - l + 1 for l, h in zip(info["lo"], info["hi"])]
    assert all(s >= 38 for s in spans) and all(l % 4 != 0 and l > 8 for l in info["lo"]) and all(h < N - 9 for h in info["hi"]), info
    smooth_and_check(renderer, "a ball of 40 cells", stored, material, fmt, rec, want, table=True)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_a_work_box_clipped_on_one_side_only(renderer, fmt):
    """33^3, a ball of 6 cells about (16.2, 15.7, 2.5): its box is cut by the face z = 0 and by no other, so the work box has its extra
    sample on five sides and the grid's own clamp on the sixth."""
    N = 33
    rng = np.random.default_rng(11)
    stored = R.dense_field(rng.uniform(-3.0, 3.0, (N, N, N)).astype(np.float32), fmt)
    material = (stored <= 0).astype(np.uint8)
    for rebound, strength, it in ((0.0, 1.0, 2), (1.0, 0.5, 1)):
        rec = v.smooth_record(_abi.BRUSH_SPHERE, (16.2, 15.7, 2.5), (0, 0, 0), 6.0, strength=strength, iterations=it, falloff=2.0, rebound=rebound,
                              material=-1)
        want = S.smooth(stored, material, fmt, rec)
        info = want[2]
        assert info["lo"][2] == 0 and info["hi"][2] < N - 2 and min(info["lo"][:2]) > 1 and max(info["hi"][:2]) < N - 2, info
        smooth_and_check(renderer, f"clipped at z = 0, rebound {rebound}", stored, material, fmt, rec, want, table=False)


def test_a_region_wholly_outside_the_grid_changes_nothing(renderer):
    N = 17
    stored, material = K.field(N, R.TEXEL16)
    rec = v.smooth_record(_abi.BRUSH_CAPSULE, (-30.0, 8.0, 8.0), (-12.0, 8.0, 8.0), 4.0, strength=1.0, iterations=2)
    want = S.smooth(stored, material, R.TEXEL16, rec)
    assert want[2]["written"] == 0
    smooth_and_check(renderer, "wholly outside", stored, material, R.TEXEL16, rec, want, table=True)


def test_the_host_mirror_follows(renderer):
    N = 17
    stored, material = K.field(N, R.F32)
    vol = K.volume(N, True)
    vol.density, vol.material_id = np.array(stored), np.array(material)
    renderer.upload_volume(EDITED, vol)
    rec = K.shape_record(N, _abi.BRUSH_BOX, strength=0.5, iterations=2, falloff=1.0, rebound=1.0, material=7)
    want_d, want_m, info = S.smooth(stored, material, R.F32, rec)
    vol.dirty = False
    got = renderer.smooth_volume(EDITED, rec, vol)
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
    call = lambda slot, rec: lib.vrt_volume_smooth(ctx, slot, rec, C.byref(res))
    assert lib.vrt_volume_smooth(None, EDITED, C.byref(good), C.byref(res)) == _abi.VRT_ERR_INVALID
    assert call(EDITED, None) == _abi.VRT_ERR_INVALID
    for slot in (7, -1, _abi.VRT_MAX_VOLUMES):
        assert call(slot, C.byref(good)) == _abi.VRT_ERR_SLOT, slot
    for what, rec in refused_records():
        assert call(EDITED, C.byref(rec)) == _abi.VRT_ERR_INVALID, what
        assert call(7, C.byref(rec)) == _abi.VRT_ERR_INVALID, what  # the record is judged before the slot
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")
    for what, rec in accepted_records():
        assert call(EDITED, C.byref(rec)) == _abi.VRT_OK, what
    assert lib.vrt_volume_smooth(ctx, EDITED, C.byref(good), None) == _abi.VRT_OK  # no result record is fine


def test_cpp_adaptor_smooths_the_demo_model(tmp_path):
    """vrt_demo --edit-smooth: every device dab into the filled red sphere is followed by a smooth record through
    VHipRenderer::SmoothVolume, before the dab's box is redistanced; the flag alone is refused."""
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out = str(tmp_path / "smoothed.ppm")
    common = [exe, "--solid", "--frames", "4", "--size", "160x90", "--out", out]
    r = subprocess.run(common + ["--edit-brush", "12", "--edit-device", "--edit-smooth", "0.5", "--sdf", "3"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("smooth:")]
    assert line and float(line[0].split()[2]) == 0.5 and int(line[0].split()[4]) > 1000, r.stdout
    assert "device brushes" in r.stdout
    r = subprocess.run(common + ["--edit-brush", "12", "--edit-smooth", "0.5"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 1 and "--edit-smooth" in r.stderr
