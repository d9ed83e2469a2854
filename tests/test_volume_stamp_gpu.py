"""vrt_volume_stamp on the device: after the call the destination's dense grid, its material ids and the result record are those of
the numpy reference of the contract (tests/stamp_ref.py), every device buffer of the destination — bricks, cell records, both levels
of the empty-space table, the Cube table and the active box — is byte-identical to a full upload of the reference's result, and every
buffer of the source reads as before.  Tolerance 0 throughout."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stamp_cases as K
import stamp_ref as S
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from test_volume_fill_gpu import EDITED, FULL, assert_same_buffers, buffers, upload_field
from test_volume_stamp import accepted_records, good_record, refused_records

pytestmark = pytest.mark.gpu
SOURCE, SPARE = 2, 5  # slots: the stamped volume; the source next to a scene's volumes


@pytest.fixture(autouse=True)
def _fresh_slots(request):
    """Tests here upload into the session renderer's slots behind SyncWithScene's back: the slots start unused and are freed after."""
    def free():
        if "renderer" in request.fixturenames:
            r = request.getfixturevalue("renderer")
            for slot in (EDITED, FULL, SOURCE, SPARE):
                r._uploaded.pop(slot, None)
                r._lib.vrt_volume_free(r._ctx, slot)  # VRT_ERR_SLOT when unused
    free()
    yield
    free()


def with_table(vol, on):
    """The volume with (step_max > 0) or without (<= 0) the empty-space tables on the device."""
    out = copy.copy(vol)
    out.step_max = 1.5 * vol.GetCellSize() if on else 0.0
    return out


def upload(r, slot, kind, N, role, fmt, table=False):
    vol = with_table(K.volume(kind, N, role), table)
    upload_field(r, slot, vol, fmt, K.stored(kind, N, role, fmt), vol.material_id)
    return vol


def check_result(got, want, what):
    assert got["written"] == want["written"], (what, got, want)
    if want["written"]:
        assert got == want, (what, got, want)
    else:
        assert all(l > h for l, h in zip(got["lo"], got["hi"])), (what, got)


def stamp_and_check(r, case, Nd, Ns, dfmt, sfmt, table):
    """Both slots uploaded, one call, then the destination against the reference and against a full upload of the reference's result,
    and the source against itself."""
    what, src_kind, dst_kind, rec = case
    what = f"{what} ({Ns}^3 fmt {sfmt} into {Nd}^3 fmt {dfmt}, tables {table})"
    dst = upload(r, EDITED, dst_kind, Nd, "dst", dfmt, table)
    upload(r, SOURCE, src_kind, Ns, "src", sfmt)
    src_before, dst_before = buffers(r, SOURCE), buffers(r, EDITED)
    want_d, want_m, want = K.reference(src_kind, dst_kind, Nd, Ns, dfmt, sfmt, rec)
    got = r.stamp_volume(EDITED, SOURCE, rec)
    check_result(got, want, what)
    have = buffers(r, EDITED)
    assert np.array_equal(have["dense"].view(np.uint32), want_d.view(np.uint32).reshape(-1)), what
    assert np.array_equal(have["material"], want_m.reshape(-1)), what
    upload_field(r, FULL, dst, dfmt, want_d, want_m)
    full = buffers(r, FULL)
    if not table:
        full["active_box"] = None  # a slot without the tables keeps whatever box it had before: not a buffer of this volume
    assert_same_buffers(have, full, what + " against a full upload")
    assert_same_buffers(buffers(r, SOURCE), src_before, what + ": the source")
    if want["written"] == 0:
        assert_same_buffers(have, dst_before, what + ": nothing written, nothing changed")
    return want


@pytest.mark.parametrize("sfmt", K.FORMATS)
@pytest.mark.parametrize("dfmt", K.FORMATS)
@pytest.mark.parametrize("Ns", [9, 17])
@pytest.mark.parametrize("Nd", [17, 33])
def test_device_stamp_equals_the_reference_over_placements_and_ops(renderer, Nd, Ns, dfmt, sfmt):
    written = {}
    for case in K.sweep(Nd, Ns):
        for table in (True, False):
            written[case[0]] = stamp_and_check(renderer, case, Nd, Ns, dfmt, sfmt, table)["written"]
    assert all(n == 0 for what, n in written.items() if what.startswith("wholly outside"))
    for name in ("identity", "shift", "axis turn 0", "axis turn 5", "oblique 0", "oblique 1", "a source larger", "u lands on"):
        assert any(n > 0 for what, n in written.items() if what.startswith(name)), name


@pytest.mark.parametrize("sfmt", K.FORMATS)
@pytest.mark.parametrize("dfmt", K.FORMATS)
def test_device_stamp_equals_the_reference_over_the_parameters(renderer, dfmt, sfmt):
    total = 0
    for n, case in enumerate(K.parameter_cross(33, 17)):
        total += stamp_and_check(renderer, case, 33, 17, dfmt, sfmt, table=n % 2 == 0)["written"]
    assert total > 5000


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_a_footprint_of_several_workgroups_and_bricks_per_axis(renderer, fmt):
    """33^3 into 65^3 at scale 1.7, oblique.  The footprint: a cube of 32 * 1.7 = 54.4 destination cells per edge covers at least that
    much of every axis however it is turned, and what the grid clips of it here still does, so the box holds more than 54^3 samples —
    hundreds of workgroups of 256 lanes, rows longer than a wave.  The written box: both fields are exact distances.  The sphere has radius
    0.62 * 16 * 1.7 = 16.864 destination cells about the placement's centre c and the torus (55 and 22 of 3.125 per cell: 17.6 and 7.04
    cells) about the grid's, |c - centre| = 2.52 cells.  The torus is nowhere below -7.04 cells, so ADD writes wherever the sphere is
    below that with some room: within 9 cells of c (-7.86).  At c the torus stands at no more than (17.6 + 2.52) - 7.04 = 13.08 cells
    and grows by at most a cell per cell, so SUBTRACT (written where d + v < 0) writes wherever (13.08 + r) + (r - 16.864) < 0 with
    some room: within 1.5 cells of c.  The smooth term only moves m further from d.  So ADD's written box spans 18 samples, five bricks,
    on every axis."""
    Nd, Ns = 65, 33
    name, matrix, scale = K.placements(Nd, Ns)[9]
    assert name.startswith("oblique 1")
    m = np.asarray(matrix, np.float64).reshape(3, 4)
    corners = np.array([[a, b, c] for a in (0, Ns - 1) for b in (0, Ns - 1) for c in (0, Ns - 1)], np.float64)
    placed = (np.linalg.inv(m[:, :3]) @ (corners - m[:, 3]).T).T  # the source's corners in destination coordinates
    assert np.all(np.minimum(placed.max(0), Nd - 1) - np.maximum(placed.min(0), 0) >= 54.4), placed
    centre = placed.mean(0)
    grid = np.stack(np.meshgrid(*[np.arange(Nd)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for op, material, radius in ((S.ADD, 7, 9.0), (S.SUBTRACT, S.SOURCE, 1.5)):
        rec = K.record(op, matrix, scale, 1.5, material, 0.0)
        want = stamp_and_check(renderer, (f"{name}, op {op}", "sphere", "torus", rec), Nd, Ns, fmt, fmt, table=True)
        ball = grid[np.linalg.norm(grid - centre, axis=1) <= radius]
        assert want["written"] >= len(ball) > 0, (want, len(ball))
        assert all(l <= b for l, b in zip(want["lo"], ball.min(0))) and all(h >= b for h, b in zip(want["hi"], ball.max(0))), want


def test_a_stamp_that_changes_nothing_leaves_every_buffer_untouched(renderer):
    Nd, Ns = 33, 17
    placed = K.placements(Nd, Ns)
    upload(renderer, EDITED, "torus", Nd, "dst", R.F32, table=True)
    upload(renderer, SOURCE, "sphere", Ns, "src", R.F32)
    before, src_before = buffers(renderer, EDITED), buffers(renderer, SOURCE)
    name, matrix, scale = placed[11]
    assert name == "wholly outside"
    for op in K.OPS:
        got = renderer.stamp_volume(EDITED, SOURCE, K.record(op, matrix, scale, 0.0, 7, 0.0))
        assert got["written"] == 0 and all(l > h for l, h in zip(got["lo"], got["hi"])), got
    assert_same_buffers(buffers(renderer, EDITED), before, "a source wholly outside")
    rec = K.record(S.SUBTRACT, placed[9][1], placed[9][2], 0.0, 0, 0.0)
    first = renderer.stamp_volume(EDITED, SOURCE, rec)
    assert first["written"] > 100
    carved = buffers(renderer, EDITED)
    second = renderer.stamp_volume(EDITED, SOURCE, rec)  # the same hard SUBTRACT again: max(d, c) == d everywhere
    assert second["written"] == 0 and all(l > h for l, h in zip(second["lo"], second["hi"])), second
    assert_same_buffers(buffers(renderer, EDITED), carved, "a second identical SUBTRACT")
    assert_same_buffers(buffers(renderer, SOURCE), src_before, "the source")


def test_a_stamp_after_an_upload_of_the_source_uses_the_new_source(renderer):
    Nd = 33
    for n, (kind, Ns, sfmt) in enumerate((("sphere", 17, R.F32), ("shell", 9, R.TEXEL16), ("hand", 17, R.F32))):
        name, matrix, scale = K.placements(Nd, Ns)[8]
        rec = K.record(S.ADD, matrix, scale, 0.0, S.SOURCE, 0.0)
        want = stamp_and_check(renderer, (f"source {n}: {kind}", kind, "torus", rec), Nd, Ns, R.F32, sfmt, table=False)
        assert want["written"] > 0


def test_refused_calls_change_nothing(renderer):
    upload(renderer, EDITED, "torus", 17, "dst", R.TEXEL16, table=True)
    upload(renderer, SOURCE, "sphere", 9, "src", R.F32)
    before, src_before = buffers(renderer, EDITED), buffers(renderer, SOURCE)
    lib, ctx = renderer._lib, renderer._ctx
    res = _abi.vrt_brush_result()
    good = good_record()
    call = lambda dst, src, rec: lib.vrt_volume_stamp(ctx, dst, src, rec, C.byref(res))
    assert lib.vrt_volume_stamp(None, EDITED, SOURCE, C.byref(good), C.byref(res)) == _abi.VRT_ERR_INVALID
    assert call(EDITED, SOURCE, None) == _abi.VRT_ERR_INVALID
    assert call(EDITED, EDITED, C.byref(good)) == _abi.VRT_ERR_INVALID and call(7, 7, C.byref(good)) == _abi.VRT_ERR_INVALID
    for dst, src in ((7, SOURCE), (EDITED, 7), (-1, SOURCE), (EDITED, -1), (_abi.VRT_MAX_VOLUMES, SOURCE), (EDITED, _abi.VRT_MAX_VOLUMES)):
        assert call(dst, src, C.byref(good)) == _abi.VRT_ERR_SLOT, (dst, src)
    for what, rec in refused_records():
        assert call(EDITED, SOURCE, C.byref(rec)) == _abi.VRT_ERR_INVALID, what
        assert call(7, SOURCE, C.byref(rec)) == _abi.VRT_ERR_INVALID, what  # the record is judged before the slots
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")
    assert_same_buffers(buffers(renderer, SOURCE), src_before, "the source after refused calls")
    for what, rec in accepted_records():
        assert call(EDITED, SOURCE, C.byref(rec)) == _abi.VRT_OK, what
    assert lib.vrt_volume_stamp(ctx, EDITED, SOURCE, C.byref(good), None) == _abi.VRT_OK  # no result record is fine


def test_a_frame_after_a_stamp_equals_a_frame_after_the_full_upload(renderer):
    sc = scenes.config3_voxelized(5, 16)
    vol = sc.volumes()[0]
    p = v.default_params(64, 36, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(p.width, p.height)
    renderer.params_override = p
    renderer.SetRendererMode(p.mode)
    untouched = renderer.Render()  # the scene's volume is resident in slot 0 now
    upload(renderer, SPARE, "sphere", 17, "src", R.F32)
    c = (vol.N - 1) / 2.0
    rec = v.stamp_from_placement(17, (c + 8.6, c, c + 1.0), K.quat((1, 1, 0), 30.0), 0.6, op=_abi.STAMP_SUBTRACT, material=0)
    got = renderer.stamp_volume(0, SPARE, rec, vol)
    assert got["written"] > 0 and vol.dirty_box is None and not vol.dirty  # the mirror follows without being dirtied
    stamped = renderer.Render()
    assert not np.array_equal(stamped, untouched)
    vol.dirty = True  # the mirror uploaded whole
    assert np.array_equal(renderer.Render(), stamped)
    renderer.params_override = None


def test_cpp_adaptor_stamps_the_demo_model(tmp_path):
    """vrt_demo --edit-stamp: the red sphere, filled, carved with a turning torus through VHipRenderer::StampVolume; the sculpted model
    leaves as a mesh."""
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out, mesh = str(tmp_path / "stamped.ppm"), str(tmp_path / "stamped.glb")
    r = subprocess.run([exe, "--solid", "--frames", "4", "--size", "160x90", "--edit-brush", "12", "--edit-stamp", "--out", out, "--mesh-out", mesh],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("stamp:")]
    assert line and int(line[0].split()[1]) == 5 and int(line[0].split()[5]) > 0, r.stdout  # the warm-up frame and four more
    assert "device stamps" in r.stdout and os.path.getsize(mesh) > 10000
