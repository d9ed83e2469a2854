"""Slot masks on the device (vrt_volume_mask_*, vrt.h) against tests/mask_ref.py on top of the session model: the mask a call leaves is
the reference's bit for bit, and after an honouring edit call on a masked slot every buffer of vrt_debug_volume_bytes equals
volume_ref.device_bytes of where(mask, before, unmasked result), the record is the unmasked run's and `restored` is the model's count.
Tolerance 0 throughout, through the `buffers` / `assert_same_buffers` of tests/test_volume_fill_gpu.py.  Every test opens a context of
its own."""
import os
import subprocess

import numpy as np
import pytest

import brush_ref as B
import extreme_cases as X
import history_ref as H
import mask_cases as MC
import mask_ref as MK
import session_model as M
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from test_volume_fill_gpu import assert_same_buffers, buffers, upload_field
from test_volume_session import same_bits
from test_volume_session_gpu import DeviceSession, check_buffers, check_record

pytestmark = pytest.mark.gpu

BIG = (1000, 1 << 40)  # history limits no test here reaches
FORMATS = (R.F32, R.TEXEL16)


def none_info(N: int, on: int = 0, restored: int = 0) -> dict:
    return {"on": on, "masked": 0, "lo": (N, N, N), "hi": (-1, -1, -1), "restored": restored}


def run_steps(r, steps, devices=(0,), session=None, before=None, restored=None):
    """The steps of mask_cases on a context: every record, every mask and its info, `restored` after every honouring call, and every
    buffer of both slots on every device after every step.  Returns (buffers per (device, slot), restored per slot) to carry on."""
    session = session or DeviceSession(r)
    before = before or {(dev, slot): None for dev in devices for slot in M.SLOTS}
    restored = {} if restored is None else restored
    for step in steps:
        kind, slot = step["kind"], step["slot"]
        what = f"step {step['n']}: {kind} on slot {slot}"
        if kind == "mask":
            got = r.mask_apply(slot, step["args"]["ops"])
            want = dict(step["want"], restored=restored.get(slot, 0))
            assert got == want == r.mask_info(slot), (what, got, want)
            assert np.array_equal(r.mask_download(slot, step["after"][slot].N), step["mask"]), what
        else:
            check_record(step, session.apply(step), what)
        if kind in ("upload", "free"):
            restored.pop(slot, None)
        if "restored" in step:
            restored[slot] = step["restored"]
            assert r.mask_info(slot)["restored"] == step["restored"], (what, r.mask_info(slot), step["restored"])
        before = check_buffers(r, step, before, what, devices)
    return before, restored


# ---- 1. the mask calls -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", (2, 5, 65, 129))
def test_the_device_mask_equals_the_reference(N, fmt):
    stored, material = X.small_field(N, fmt)  # NaN and +-0 samples among them: SOLID in both formats
    ref = MC.reference(N, fmt)
    MC.check_cases_are_what_they_say(N, ref)
    with v.VHipRenderer(devices=(0,)) as r:
        upload_field(r, 0, X.volume(N, fmt, False), fmt, stored, material)
        assert r.mask_info(0) == none_info(N) and not r.mask_download(0, N).any()
        held = buffers(r, 0)
        for name, ops in MC.cases(N):
            r.mask_clear(0)
            got = r.mask_apply(0, ops)
            assert got == MK.info(ref[name]) == r.mask_info(0), (name, got, MK.info(ref[name]))
            have = r.mask_download(0, N)
            assert np.array_equal(have, ref[name]), (name, int((have != ref[name]).sum()))
        # one call of n records leaves what n calls of one record leave
        r.mask_clear(0)
        for op in dict(MC.cases(N))["a sequence"]:
            r.mask_apply(0, [op])
        assert np.array_equal(r.mask_download(0, N), ref["a sequence"])
        # an upload of bytes other than 0 / 1 downloads as 0 / 1, over the mask that was there
        rng = np.random.default_rng(N)
        raw = rng.integers(0, 4, (N, N, N)).astype(np.uint8) * rng.integers(1, 86, (N, N, N)).astype(np.uint8)
        raw[0, 0, 0], raw[N - 1, N - 1, N - 1] = 255, 2
        assert raw[0, 0, 0] == 255 and raw[N - 1, N - 1, N - 1] == 2  # bytes that a test for `== 1` or for `& 1` would get wrong
        _abi.check(r._lib.vrt_volume_mask_upload(r._ctx, 0, raw.ctypes.data), "vrt_volume_mask_upload")  # the bytes as they are
        assert r.mask_info(0) == MK.info(raw != 0)
        out = np.zeros((N, N, N), np.uint8)
        _abi.check(r._lib.vrt_volume_mask_download(r._ctx, 0, out.ctypes.data), "vrt_volume_mask_download")
        assert set(np.unique(out)) <= {0, 1} and np.array_equal(out != 0, raw != 0)
        r.mask_clear(0)
        r.mask_clear(0)  # fine on a slot without one
        assert r.mask_info(0) == none_info(N) and r.mask_apply(0, []) == none_info(N, on=1)
        assert_same_buffers(buffers(r, 0), held, "the mask calls write nothing to the volume")


def test_the_mask_calls_refuse_what_the_header_says():
    stored, material = X.small_field(3, R.F32)
    with v.VHipRenderer(devices=(0,)) as r:
        lib, ctx = r._lib, r._ctx
        info = _abi.vrt_mask_info()
        one = (_abi.vrt_mask_op * 1)(MK.op(MK.ALL, 1))
        assert lib.vrt_volume_mask_apply(ctx, 0, 1, one, None) == _abi.VRT_ERR_SLOT
        assert lib.vrt_volume_mask_info(ctx, 0, info) == _abi.VRT_ERR_SLOT and lib.vrt_volume_mask_clear(ctx, 0) == _abi.VRT_ERR_SLOT
        assert lib.vrt_volume_mask_clear(ctx, -1) == _abi.VRT_ERR_SLOT
        upload_field(r, 0, X.volume(3, R.F32, False), R.F32, stored, material)
        r.mask_apply(0, [MC.slab(3, 0, 0)])
        want = r.mask_download(0, 3)
        for what, ops in MC.refused_records():
            arr = (_abi.vrt_mask_op * len(ops))(*ops)
            assert lib.vrt_volume_mask_apply(ctx, 0, len(ops), arr, info) == _abi.VRT_ERR_INVALID, what
        assert lib.vrt_volume_mask_apply(ctx, 0, 1, None, info) == _abi.VRT_ERR_INVALID
        assert lib.vrt_volume_mask_upload(ctx, 0, None) == _abi.VRT_ERR_INVALID and lib.vrt_volume_mask_download(ctx, 0, None) == _abi.VRT_ERR_INVALID
        assert lib.vrt_volume_mask_info(ctx, 0, None) == _abi.VRT_ERR_INVALID
        assert np.array_equal(r.mask_download(0, 3), want) and want.sum() == 9


# ---- 2. the seven honouring calls --------------------------------------------------------------------------------------------------------

def assert_not_vacuous(step, what):
    """From the model alone, before the device is asked."""
    assert step["restored"] > 0, (what, "the call changes no protected sample")
    assert step["unprotected"] > 0, (what, "the call changes no unprotected sample")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", MC.HONOURING)
def test_an_honouring_call_leaves_protected_samples_alone(kind, fmt):
    steps = MC.edit_case(kind, fmt)  # N = 33, the tables on
    assert steps[-1]["kind"] == kind and steps[-1]["after"][0].tables
    assert_not_vacuous(steps[-1], kind)
    with v.VHipRenderer(devices=(0,)) as r:
        run_steps(r, steps)


def brush_case_65(fmt):
    """A dab across y = 60 on 65^3, where the samples y >= 60 are protected: the put-back's words 0 and 1 of a row, the second with
    its one live bit."""
    g = M._Generator(77, (fmt,))
    g.upload(1, 2, fmt)
    g.upload(0, 6, fmt)
    g.set_metric(0, True)
    masks = {}
    MC.mask_step(g, masks, 0, [MC.slab(65, 60, 64)])
    MC.honour(g, masks, 0, lambda: g._brushes(0, [v.sphere_brush(B.ADD, (32.3, 60.2, 31.6), 7.5, 0.0, 2.0, 5)]))
    return tuple(g.steps)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_brush_across_the_word_boundary_of_65_cubed(fmt):
    steps = brush_case_65(fmt)
    assert_not_vacuous(steps[-1], "the dab")
    before, after = steps[-2]["after"][0], steps[-1]["after"][0]
    changed = MK.bits(before.stored) != MK.bits(after.stored)
    assert changed[:, :, :60].any() and not changed[:, :, 60:].any() and steps[-1]["want"]["hi"][1] == 64
    with v.VHipRenderer(devices=(0,)) as r:
        run_steps(r, steps)


def test_an_honouring_call_over_two_devices():
    steps = MC.edit_case("smooth", R.TEXEL16)
    assert_not_vacuous(steps[-1], "smooth")
    with v.VHipRenderer(devices=(0, 0)) as r:
        run_steps(r, steps, devices=(0, 1))


# ---- 3. and 4. what writes through, and the history ---------------------------------------------------------------------------------------

def small_program(fmt, res=4):
    """Slot 0 (17^3, the tables on) and the stamp's source in slot 1, ready for edits; the generator carries on."""
    g = M._Generator(83, (fmt,))
    g.upload(1, 2, fmt)
    g.upload(0, res, fmt)
    g.set_metric(0, True)
    return g


def state_of(m):
    return m.stored, m.material


@pytest.mark.parametrize("fmt", FORMATS)
def test_updates_undo_and_redo_write_through_the_mask(fmt):
    g = small_program(fmt)
    masks = {}
    MC.honour(g, masks, 0, lambda: g.brushes(0))  # an edit before the mask is painted
    unmasked_edit = g.steps[-1]
    assert unmasked_edit["restored"] == 0 and unmasked_edit["unprotected"] > 0
    MC.mask_step(g, masks, 0, [MK.op(MK.ALL, 1)])
    n_all = len(g.steps)
    g.update_region(0, records=True)  # over protected samples: lands
    MC.mask_step(g, masks, 0, [MK.op(MK.ALL, 0), MC.z_half(17)])
    MC.honour(g, masks, 0, lambda: g.smooth(0, small=False))
    masked_edit = g.steps[-1]
    assert_not_vacuous(masked_edit, "smooth")
    steps = tuple(g.steps)
    hist = H.History(*BIG)
    with v.VHipRenderer(devices=(0,)) as r:
        session = DeviceSession(r)
        before, restored = run_steps(r, steps[:3], session=session)
        r.enable_history(0, *BIG)
        start = before[(0, 0)]
        before, restored = run_steps(r, steps[3:n_all], session=session, before=before, restored=restored)
        assert hist.record(state_of(steps[2]["after"][0]), state_of(unmasked_edit["after"][0])) > 0
        # an undo of an edit made before the mask was painted changes protected samples; the redo brings them back
        r.undo(0, 1)
        assert_same_buffers(buffers(r, 0), start, "the undo through a mask of everything")
        r.redo(0, 1)
        assert_same_buffers(buffers(r, 0), before[(0, 0)], "the redo through a mask of everything")
        assert r.mask_info(0)["masked"] == 17 ** 3
        before, restored = run_steps(r, steps[n_all:-1], session=session, before=before, restored=restored)  # the update lands
        update = steps[n_all]
        assert update["kind"] == "update_region" and hist.record(state_of(steps[n_all - 1]["after"][0]), state_of(update["after"][0])) > 0
        held = before[(0, 0)]
        before, restored = run_steps(r, steps[-1:], session=session, before=before, restored=restored)
        # the entry of the masked edit: the tiles that differ after the put-back
        tiles = hist.record(state_of(steps[-2]["after"][0]), state_of(masked_edit["after"][0]))
        assert tiles > 0 and r.history_info(0) == hist.info(), (r.history_info(0), hist.info())
        r.undo(0, 1)
        assert_same_buffers(buffers(r, 0), held, "the undo of a masked edit")
        r.redo(0, 1)
        assert_same_buffers(buffers(r, 0), before[(0, 0)], "the redo of a masked edit")
        assert np.array_equal(r.mask_download(0, 17), masks[0])  # neither changes the mask


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_masked_edit_that_changes_nothing_records_nothing(fmt):
    g = small_program(fmt)
    MC.honour(g, {}, 0, lambda: g.brushes(0))
    assert g.steps[-1]["unprotected"] > 0
    steps = tuple(g.steps)
    g2, masks = small_program(fmt), {}  # the same slot without the brush: what the undo leaves
    MC.mask_step(g2, masks, 0, [MK.op(MK.ALL, 1)])
    MC.honour(g2, masks, 0, lambda: g2.smooth(0, small=False))  # everything it touches is protected
    smooth = g2.steps[-1]
    assert smooth["restored"] > 0 and smooth["unprotected"] == 0 and smooth["want"]["written"] > 0
    with v.VHipRenderer(devices=(0,)) as r:
        session = DeviceSession(r)
        before, restored = run_steps(r, steps[:3], session=session)
        r.enable_history(0, *BIG)
        run_steps(r, steps[3:], session=session, before=before, restored=restored)
        r.undo(0, 1)  # the slot is as before the brush, with one redo entry
        info = r.history_info(0)
        assert (info["undo_entries"], info["redo_entries"]) == (0, 1)
        undone = buffers(r, 0)
        assert r.mask_apply(0, [MK.op(MK.ALL, 1)])["masked"] == 17 ** 3
        rec = r.smooth_volume(0, smooth["args"]["record"])
        assert M.same_record("smooth", rec, smooth["want"]) and rec["written"] > 0
        assert r.mask_info(0)["restored"] == smooth["restored"]
        assert_same_buffers(buffers(r, 0), undone, "an edit of a wholly protected slot")
        assert r.history_info(0) == info  # nothing recorded, the redo stack kept


# ---- 5. lifetime and isolation -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_uploads_and_free_drop_the_mask_and_slots_do_not_share_one(fmt):
    g = small_program(fmt)
    masks = {}
    MC.mask_step(g, masks, 1, [MK.op(MK.ALL, 1)])      # the stamp's source wholly protected: ignored
    MC.honour(g, {}, 0, lambda: g.stamp(0, 1))          # ... and slot 0 has no mask: the edit is unmasked
    assert g.steps[-1]["unprotected"] > 0
    MC.mask_step(g, masks, 0, [MK.op(MK.ALL, 1), MK.op(MK.ALL, 0)])  # a mask without a set bit: as no mask
    MC.honour(g, masks, 0, lambda: g.brushes(0))
    assert g.steps[-1]["restored"] == 0 and g.steps[-1]["unprotected"] > 0
    MC.mask_step(g, masks, 0, [MK.op(MK.ALL, 1)])
    g.upload(0, 4, fmt)                                 # drops the mask
    masks.pop(0)
    g.set_metric(0, True)
    n_upload = len(g.steps)
    MC.honour(g, masks, 0, lambda: g.brushes(0))        # unmasked again
    assert g.steps[-1]["unprotected"] > 0
    MC.mask_step(g, masks, 0, [MK.op(MK.ALL, 1)])
    g.free(0)
    masks.pop(0)
    n_free = len(g.steps)
    g.upload(0, 3, fmt)
    MC.honour(g, masks, 0, lambda: g.brushes(0))
    assert g.steps[-1]["unprotected"] > 0
    steps = tuple(g.steps)
    with v.VHipRenderer(devices=(0,)) as r:
        session = DeviceSession(r)
        state = run_steps(r, steps[:n_upload], session=session)
        assert r.mask_info(0) == none_info(17) and not r.mask_download(0, 17).any()
        assert r.mask_info(1)["masked"] == 5 ** 3       # slot 1 keeps its own
        state = run_steps(r, steps[n_upload:n_free], session=session, before=state[0], restored=state[1])
        info = _abi.vrt_mask_info()
        assert r._lib.vrt_volume_mask_info(r._ctx, 0, info) == _abi.VRT_ERR_SLOT
        run_steps(r, steps[n_free:], session=session, before=state[0], restored=state[1])
        assert r.mask_info(0) == none_info(9)


# ---- 6. a sequence with carried state ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp,fq", [(R.F32, R.TEXEL16), (R.TEXEL16, R.F32)])
def test_a_sequence_of_mask_records_and_honouring_edits_on_two_slots(fp, fq):
    steps = MC.sequence(fp, fq)
    alternating = [s for s in steps if s["kind"] == "mask" or "restored" in s]
    assert len(alternating) >= 12 and all((a["kind"] == "mask") != (b["kind"] == "mask") for a, b in zip(alternating, alternating[1:]))
    edits = [s for s in alternating if "restored" in s]
    assert sum(s["restored"] > 0 and s["unprotected"] > 0 for s in edits) >= 5 and {s["slot"] for s in edits} == {0, 1}
    with v.VHipRenderer(devices=(0,)) as r:
        run_steps(r, steps)


# ---- 7. extremes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_resolution_0(fmt):
    g = M._Generator(5, (fmt,))
    g.upload(1, 2, fmt)
    g.upload(0, 0, fmt)
    g.set_metric(0, True)
    masks = {}
    MC.mask_step(g, masks, 0, [MC.slab(2, 0, 0), MK.op(MK.GROW, steps=1), MK.op(MK.SHRINK, steps=1), MK.op(MK.INVERT), MK.op(MK.INVERT),
                               MC.slab(2, 1, 1, 0)])
    assert masks[0].sum() == 4
    MC.honour(g, masks, 0, lambda: g._brushes(0, [v.sphere_brush(B.ADD, (0.5, 0.5, 0.5), 3.0, 0.0, 2.0, 4)]))
    assert_not_vacuous(g.steps[-1], "the dab on 2^3")
    with v.VHipRenderer(devices=(0,)) as r:
        run_steps(r, tuple(g.steps))


def test_resolution_9():
    """N = 513, nine words per row: one SHAPE record that reaches the row's last word and its one live bit (y = 512), one dab across
    the shape's boundary.  Both act inside the samples 240..272 x 480..512 x 240..272, so the model is a 33^3 grid holding that box:
    the shapes' centres have few fraction bits and p - a is the same float there as here, and its cell size is the same 2.0."""
    N, n, O = 513, 33, (240, 480, 240)
    shift = lambda p: tuple(a - o for a, o in zip(p, O))
    at_mask, at_dab = (256.5, 506.25, 256.25), (262.5, 504.25, 256.25)
    assert B.units(N, 512.0, 1.0) == B.units(n, 32.0, 1.0)
    stored, material = np.full((n, n, n), 30.0, np.float32), np.zeros((n, n, n), np.uint8)
    mask = MK.apply(None, [MK.op(MK.SHAPE, 1, _abi.BRUSH_SPHERE, a=shift(at_mask), radius=8.5)], stored, material, R.F32)
    d, m = stored.copy(), material.copy()
    want = B.apply(d, m, R.F32, [v.sphere_brush(B.ADD, shift(at_dab), 7.0, 0.0, 2.0, 3)], 32.0, 1.0)
    wrote = (MK.bits(d) != MK.bits(stored)) | (m != material)
    for a in (mask, wrote):  # nothing reaches the model's faces but the one it shares with the grid
        assert not (a[0].any() or a[-1].any() or a[:, 0].any() or a[:, -1].any() or a[:, :, 0].any()) and a[:, :, -1].any()
    want_d, want_m, restored = MK.protect(mask, stored, material, d, m)
    assert restored > 0 and int((MK.bits(want_d) != MK.bits(stored)).sum()) > 0
    big = X.volume(N, R.F32, False, extent=512.0, scale=1.0)
    with v.VHipRenderer(devices=(0,)) as r:
        upload_field(r, 0, big, R.F32, np.full((N, N, N), 30.0, np.float32), np.zeros((N, N, N), np.uint8))
        info, ref = r.mask_apply(0, [MK.op(MK.SHAPE, 1, _abi.BRUSH_SPHERE, a=at_mask, radius=8.5)]), MK.info(mask)
        assert info["masked"] == ref["masked"] and info["hi"][1] == N - 1
        assert info["lo"] == tuple(a + o for a, o in zip(ref["lo"], O)) and info["hi"] == tuple(a + o for a, o in zip(ref["hi"], O))
        got = r.apply_brushes(0, None, [v.sphere_brush(B.ADD, at_dab, 7.0, 0.0, 2.0, 3)])
        assert got["written"] == want["written"] and got["lo"] == tuple(a + o for a, o in zip(want["lo"], O))
        assert got["hi"] == tuple(a + o for a, o in zip(want["hi"], O))
        assert r.mask_info(0) == dict(info, restored=restored)
        have_d, have_m = r.download_region(0, O, tuple(o + n - 1 for o in O))
        assert same_bits(have_d, want_d) and np.array_equal(have_m, want_m)
        outside_d, outside_m = r.download_region(0, (230, 470, 230), (239, 512, 280))
        assert (outside_d == np.float32(30.0)).all() and not outside_m.any()


# ---- the C++ adaptor ---------------------------------------------------------------------------------------------------------------------

def test_cpp_adaptor_masks_the_demo_model(tmp_path):
    """vrt_demo --edit-mask: half of the red sphere's volume is protected through VHipRenderer::MaskVolume ahead of the first device
    dab, and the mask is still there, with its count, after the last; the flag without a device-side edit is refused."""
    exe =os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    common = [exe, "--frames", "4", "--size", "160x90", "--out", str(tmp_path / "masked.ppm")]
    r = subprocess.run(common + ["--edit-brush", "12", "--edit-device", "--edit-mask"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("mask:")]
    assert len(lines) == 2 and lines[0][4] == "x" and lines[0][5].startswith("0.."), r.stdout
    protected, last_x = int(lines[0][1]), int(lines[0][-1].split("..")[1])
    N = 2 * (last_x + 1) + 1
    assert protected == N * N * (last_x + 1) and lines[1][1:4] == ["on", "1,", str(protected)], r.stdout
    assert "device brushes" in r.stdout
    r = subprocess.run(common + ["--edit-brush", "12", "--edit-mask"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 1 and "--edit-mask" in r.stderr
