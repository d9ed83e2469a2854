"""The edit history on the device (vrt_volume_history / _history_info / _undo / _redo, vrt.h) against tests/history_ref.py on top of the
session model: an undo leaves every buffer of vrt_debug_volume_bytes exactly as it was before the recorded call, a redo exactly as it was
after it, and the reported entries, tiles and bytes are the model's.  Tolerance 0 throughout, through the `buffers` /
`assert_same_buffers` of tests/test_volume_fill_gpu.py.  Every test opens a context of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brush_ref as B
import components_ref as CR
import extreme_cases as X
import history_ref as H
import session_model as M
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from test_volume_fill_gpu import STAT_KEYS, assert_same_buffers, buffers, upload_field, volume_case
from test_volume_session import F32_SEED, SEEDS, same_bits, what_of
from test_volume_session_gpu import DeviceSession, check_buffers, check_record, frame_params, set_frame

pytestmark = pytest.mark.gpu

BIG = (1000, 1 << 40)  # limits no test here reaches unless it sets its own
EDITED, OTHER = 0, 1


def state_of(m):
    return m.stored, m.material


def check_info(r, slot, hist, what):
    got = r.history_info(slot)
    want = hist.info() if hist is not None else dict.fromkeys(got, 0)
    assert got == want, (what, got, want)


def undo_and_redo(r, slot, hist, m_after, before, after, what, devices=(0,), others=()):
    """One undo: every buffer as `before`; one redo: every buffer as `after`, which the caller has held to the model.  The results and
    the info are the model's; the slots of `others` (slot -> buffers per device) stay byte-identical."""
    d, m, want = hist.undo_steps(state_of(m_after), 1)
    got = r.undo(slot, 1)
    assert got == want, (what, "undo", got, want)
    for dev in devices:
        assert_same_buffers(buffers(r, slot, dev), before[dev], f"{what}: after undo, device {dev}, against what it was before the call")
        for other, held in others:
            assert_same_buffers(buffers(r, other, dev), held[dev], f"{what}: slot {other} after an undo on slot {slot}")
    check_info(r, slot, hist, what + " after undo")
    d, m, want = hist.redo_steps((d, m), 1)
    assert same_bits(d, m_after.stored) and np.array_equal(m, m_after.material)
    got = r.redo(slot, 1)
    assert got == want, (what, "redo", got, want)
    for dev in devices:
        assert_same_buffers(buffers(r, slot, dev), after[dev], f"{what}: after redo, device {dev}, against what it was after the call")
        for other, held in others:
            assert_same_buffers(buffers(r, other, dev), held[dev], f"{what}: slot {other} after a redo on slot {slot}")
    check_info(r, slot, hist, what + " after redo")


def run_with_history(r, seed, steps, devices=(0,)):
    """The steps of a program with the history on for both slots.  Returns how many steps recorded an entry."""
    session = DeviceSession(r)
    hist = {slot: None for slot in M.SLOTS}
    before = {(dev, slot): None for dev in devices for slot in M.SLOTS}
    models = (M.SlotModel(), M.SlotModel())
    recorded = 0
    for step in steps:
        what = what_of(seed, step)
        kind, slot = step["kind"], step["slot"]
        got = session.apply(step)
        check_record(step, got, what)
        now = check_buffers(r, step, before, what, devices)
        m_before, m_after = models[slot], step["after"][slot]
        if kind == "free":
            hist[slot] = None
        elif kind == "upload":
            if hist[slot] is None:  # into an unused slot: the history is turned on (again)
                r.enable_history(slot, *BIG)
                hist[slot] = H.History(*BIG)
            else:
                hist[slot].clear()
        elif kind in M.EDITS and hist[slot].record(state_of(m_before), state_of(m_after)):
            recorded += 1
            check_info(r, slot, hist[slot], what)
            other = 1 - slot
            others = [(other, {dev: now[(dev, other)] for dev in devices})] if step["after"][other].used else []
            undo_and_redo(r, slot, hist[slot], m_after, {dev: before[(dev, slot)] for dev in devices}, {dev: now[(dev, slot)] for dev in devices},
                          what, devices, others)
        for s in M.SLOTS:
            if step["after"][s].used:
                check_info(r, s, hist[s], what)
        before, models = now, step["after"]
    return recorded


SESSIONS = [(SEEDS[0], {}), (F32_SEED, {"formats": (R.F32,)}), (SEEDS[1], {"formats": (R.TEXEL16,)})]


@pytest.mark.parametrize("seed,kw", SESSIONS)
def test_every_recording_step_of_a_session_can_be_undone_and_redone(seed, kw):
    steps = M.program(seed, **kw)
    with v.VHipRenderer(devices=(0,)) as r:
        recorded = run_with_history(r, seed, steps)
    writes = sum(s["kind"] in M.EDITS and M.wrote(s["kind"], s["want"]) for s in steps)
    print(f"seed {seed}: {recorded} of {writes} writing steps recorded an entry")
    assert recorded >= 15


def test_a_session_with_history_over_two_devices():
    with v.VHipRenderer(devices=(0, 0)) as r:
        assert run_with_history(r, SEEDS[0], M.program(SEEDS[0]), devices=(0, 1)) >= 15


# ---- each call kind on its own, at the grids where tiling can go wrong ----------------------------------------------------------------

def kinds_program(res: int, fmt: int):
    """A program whose every edit follows a fresh upload of slot 0 (slot 1 holds the stamp's 5^3 source): the eight kinds, one by one."""
    g = M._Generator(50 + res, (fmt,))
    N = (1 << res) + 1

    def fresh():
        g.upload(0, res, fmt)
        g.set_metric(0, True)

    g.upload(1, 2, fmt)
    for edit in (lambda: g.update_region(0, records=False), lambda: g.update_region(0, records=True), lambda: g.brushes(0),
                 lambda: g.stamp(0, 1), lambda: g.smooth(0, small=False), lambda: g.warp(0, small=False),
                 lambda: g.components(0, CR.REMOVE_SMALL), lambda: g.redistance(0, whole=True)):
        fresh()
        edit()
    # the fill: solid with the samples that lie on no face hollow (nothing to enclose at N = 2)
    sealed = X.fill_fields(N)["sealed"][0]
    args = dict(res=res, extent=M.EXTENTS[0], fmt=fmt, path="float", density=M._frozen(sealed, np.float32),
                material=M._frozen(np.zeros((N, N, N), np.uint8), np.uint8))
    new = g.m[0].copy()
    new.upload(**args)
    g.step("upload", 0, None, new, **args)
    g.fill(0)
    return tuple(g.steps)


@pytest.mark.parametrize("fmt", X.FORMATS)
@pytest.mark.parametrize("res", [0, 1, 3, 4])  # N = 2, 3: every tile is partial; 9: one full tile and a last tile one sample thick; 17
def test_each_call_kind_on_its_own(res, fmt):
    steps = kinds_program(res, fmt)
    with v.VHipRenderer(devices=(0,)) as r:
        recorded = run_with_history(r, f"kinds at resolution {res}", steps)
    print(f"resolution {res}, format {fmt}: {recorded} of 9 edits recorded an entry")
    assert recorded >= (7 if res >= 3 else 3)


@pytest.mark.parametrize("fmt", X.FORMATS)
@pytest.mark.parametrize("res", [1, 3])  # N = 3: every tile is partial; 9: one full tile and a last tile one sample thick
def test_each_call_kind_on_its_own_over_two_devices(res, fmt):
    """The context is fresh, so every scratch and history buffer of both devices is allocated by the first call of its kind: each call
    has to have all of them, on both devices, before it writes a sample on either."""
    steps = kinds_program(res, fmt)
    with v.VHipRenderer(devices=(0, 0)) as r:
        recorded = run_with_history(r, f"kinds at resolution {res}, two devices", steps, devices=(0, 1))
    print(f"resolution {res}, format {fmt}, two devices: {recorded} of 9 edits recorded an entry")
    assert recorded >= (7 if res >= 3 else 3)


def test_a_whole_grid_fill_of_65_cubed():
    """4913 tiles in the grid, of which the fill's written box meets hundreds: many workgroups of four waves, one wave per tile."""
    case = volume_case("6", _abi.FORMAT_F32)
    hist = H.History(*BIG)
    tiles = hist.record((case.stored, case.material), (case.want_d, case.want_m))
    box_tiles = int(np.prod([hi // H.TILE - lo // H.TILE + 1 for lo, hi in zip(case.info["lo"], case.info["hi"])]))
    print(f"the fill of 65^3 changes {tiles} of the {box_tiles} tiles its box meets")
    assert box_tiles > tiles > 256
    with v.VHipRenderer(devices=(0,)) as r:
        upload_field(r, EDITED, case.vol, case.fmt, case.stored, case.material)
        r.enable_history(EDITED, *BIG)
        before = buffers(r, EDITED)
        got = r.fill_enclosed(EDITED, None, case.wall, case.material_id)
        assert got["filled"] == case.info["filled"]
        after = buffers(r, EDITED)
        assert_same_buffers(after, case.device_bytes(), "the fill with the history on")
        check_info(r, EDITED, hist, "the fill of 65^3")
        after_model = M.SlotModel()
        after_model.stored, after_model.material = case.want_d, case.want_m
        undo_and_redo(r, EDITED, hist, after_model, {0: before}, {0: after}, "the fill of 65^3")


# ---- bits --------------------------------------------------------------------------------------------------------------------------------

def slot_model(res, extent, fmt, stored, material, scale=1.0, step=0.0):
    m = M.SlotModel()
    m.used, m.res, m.N, m.extent, m.fmt = True, res, (1 << res) + 1, float(extent), fmt
    m._set(stored, material)
    m.set_metric(scale, step)
    return m


def upload_model(r, slot, m):
    vol = v.VVoxelVolume(m.res, m.extent)
    vol.density_scale, vol.step_max = m.scale, m.step
    upload_field(r, slot, vol, m.fmt, np.array(m.stored), np.array(m.material))


def dense_bits(r, slot):
    return buffers(r, slot)["dense"].view(np.uint32)


def test_texel16_undo_is_lossless_where_download_and_update_are_not():
    res, N, extent = 4, 17, 100.0
    q = np.full((N, N, N), 300.0, np.float32)  # +-q as the slot stores it: 3.00 everywhere ...
    for i, value in enumerate((5, 10, 15, 20, 23)):  # ... but the values that a decode and an encode move down by one
        q[7 + i % 3, 8, 7 + i] = np.float32(value)
    m0 = slot_model(res, extent, R.TEXEL16, q, np.zeros((N, N, N), np.uint8), 1.0, 20.0)
    brush = [v.sphere_brush(B.ADD, (8.2, 9.0, 8.1), 3.5, 0.0, 2.0, 4)]
    m1 = m0.copy()
    want = m1.brushes(brush)
    assert want["written"] > 50 and all(lo <= 7 and hi >= 11 for lo, hi in zip(want["lo"], want["hi"]))
    hist = H.History(*BIG)
    assert hist.record(state_of(m0), state_of(m1)) > 0
    with v.VHipRenderer(devices=(0,)) as r:
        upload_model(r, EDITED, m0)
        original = buffers(r, EDITED)
        assert np.array_equal(original["dense"].view(np.float32), q.reshape(-1))
        r.enable_history(EDITED, *BIG)
        lo, hi = want["lo"], want["hi"]
        held = r.download_region(EDITED, lo, hi)  # the only way back there is without a history: the box, decoded
        assert r.apply_brushes(EDITED, None, brush) == want
        assert_same_buffers(buffers(r, EDITED), m1.expected_buffers(), "after the brush")
        check_info(r, EDITED, hist, "after the brush")
        assert r.undo(EDITED) == hist.undo_steps(state_of(m1))[2]
        assert_same_buffers(buffers(r, EDITED), original, "after undo")
        assert np.array_equal(dense_bits(r, EDITED), H.bits_of(q).reshape(-1))
        # the control: the same box downloaded before the edit and written back after it does NOT restore the bits
        r.redo(EDITED)
        vol = v.VVoxelVolume(res, extent)
        vol.density, vol.material_id = np.zeros((N, N, N), np.float32), np.zeros((N, N, N), np.uint8)
        at = (slice(lo[0], hi[0] + 1), slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1))
        vol.density[at], vol.material_id[at] = held
        r.update_volume_region(EDITED, vol, lo, hi)
        lossy = dense_bits(r, EDITED)
        wrong = np.flatnonzero(lossy != H.bits_of(q).reshape(-1))
        print(f"download + update_region left {wrong.size} samples off their bits")
        assert wrong.size >= 5 and set(lossy.view(np.float32)[wrong]) <= {4.0, 9.0, 14.0, 19.0, 22.0}
        assert r.history_info(EDITED)["undo_entries"] == 2  # that update changed bits too: it is an entry like any other


def special_field():
    N = 9
    rng = np.random.default_rng(3)
    d = rng.standard_normal((N, N, N)).astype(np.float32)
    d[2, 3, 4], d[3, 3, 3], d[4, 5, 3] = np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf)
    d.view(np.uint32)[3, 4, 4] = 0x7FC12345   # a quiet NaN with a payload
    d.view(np.uint32)[8, 8, 8] = 0xFFA00001   # a negative one, with another, in the last tile
    return d, rng.integers(0, 200, (N, N, N)).astype(np.uint8)


def test_special_values_survive_undo_and_redo_in_bits():
    d, ids = special_field()
    m0 = slot_model(3, 60.0, R.F32, d, ids, 1.0, 12.0)
    m1 = m0.copy()
    m1.update_region((2, 3, 3), np.full((3, 2, 2), 0.25, np.float32), None)   # over -0, +inf and the NaN; x 2..4, z 3..4, y 3..4
    m2 = m1.copy()
    m2.update_region((4, 0, 0), np.full((5, 9, 9), -0.5, np.float32), np.full((5, 9, 9), 7, np.uint8))  # over -inf and the last tile
    hist = H.History(*BIG)
    with v.VHipRenderer(devices=(0,)) as r:
        upload_model(r, EDITED, m0)
        assert np.array_equal(dense_bits(r, EDITED), H.bits_of(d).reshape(-1)), "the upload keeps the bits"
        r.enable_history(EDITED, *BIG)
        session = DeviceSession(r)
        session._update(EDITED, dict(origin=(2, 3, 3), values=np.full((3, 2, 2), 0.25, np.float32), material=None, records=False))
        hist.record(state_of(m0), state_of(m1))
        session._update(EDITED, dict(origin=(4, 0, 0), values=np.full((5, 9, 9), -0.5, np.float32), material=np.full((5, 9, 9), 7, np.uint8),
                                    records=True))
        hist.record(state_of(m1), state_of(m2))
        after = buffers(r, EDITED)
        assert_same_buffers(after, m2.expected_buffers(), "after both updates")
        check_info(r, EDITED, hist, "after both updates")
        _, _, want = hist.undo_steps(state_of(m2), 2)
        assert r.undo(EDITED, 2) == want
        assert_same_buffers(buffers(r, EDITED), m0.expected_buffers(), "after undo 2")
        assert np.array_equal(dense_bits(r, EDITED), H.bits_of(d).reshape(-1)), "payloads, infinities and the sign of zero"
        _, _, want = hist.redo_steps(state_of(m0), 2)
        assert r.redo(EDITED, 2) == want
        assert_same_buffers(buffers(r, EDITED), after, "after redo 2")
        r.undo(EDITED, 1)
        assert_same_buffers(buffers(r, EDITED), m1.expected_buffers(), "after undo 1: the specials under the second update are back")


# ---- depth, limits, lifetime -------------------------------------------------------------------------------------------------------------

def dab_models(fmt=R.F32, n=5, res=4):
    """A 17^3 sphere and n SUBTRACT dabs along its surface: the models after 0..n dabs, and the dabs."""
    N = (1 << res) + 1
    d, ids = M.analytic_field(np.random.default_rng(11), N, 100.0, "sphere")
    models = [slot_model(res, 100.0, fmt, R.dense_field(d, fmt), ids, 1.0, 18.0)]
    dabs = []
    c = (N - 1) / 2.0
    for i in range(n):
        a = 2.0 * np.pi * i / n
        dabs.append([v.sphere_brush(B.SUBTRACT, (c + 5.0 * np.cos(a), c + 5.0 * np.sin(a), c + 0.3 * i), 2.0, 0.0, 2.0, 0)])
        m = models[-1].copy()
        assert m.brushes(dabs[-1])["written"] > 0
        models.append(m)
    return models, dabs


def test_depth_undo_three_redo_two_undo_four_and_a_new_edit():
    models, dabs = dab_models()
    hist = H.History(*BIG)
    with v.VHipRenderer(devices=(0,)) as r:
        upload_model(r, EDITED, models[0])
        r.enable_history(EDITED, *BIG)
        held = [buffers(r, EDITED)]
        for i, dab in enumerate(dabs):
            r.apply_brushes(EDITED, None, dab)
            assert hist.record(state_of(models[i]), state_of(models[i + 1])) > 0
            held.append(buffers(r, EDITED))
            assert_same_buffers(held[-1], models[i + 1].expected_buffers(), f"after dab {i}")
        at = 5
        for call, k in (("undo", 3), ("redo", 2), ("undo", 4)):
            d, m, want = (hist.undo_steps if call == "undo" else hist.redo_steps)(state_of(models[at]), k)
            at += -k if call == "undo" else k
            assert same_bits(d, models[at].stored)
            got = getattr(r, call)(EDITED, k)
            assert got == want and want["written"] > 0, (call, k, got, want)
            assert_same_buffers(buffers(r, EDITED), held[at], f"after {call} {k}: the buffers after dab {at - 1}")
            check_info(r, EDITED, hist, f"after {call} {k}")
        assert at == 0 and r.history_info(EDITED)["redo_entries"] == 5
        # a new edit after an undo empties the redo stack
        r.apply_brushes(EDITED, None, dabs[2])
        m = models[0].copy()
        m.brushes(dabs[2])
        hist.record(state_of(models[0]), state_of(m))
        check_info(r, EDITED, hist, "after a new edit")
        assert r.history_info(EDITED)["redo_entries"] == 0
        now = buffers(r, EDITED)
        res = _abi.vrt_brush_result()
        assert r._lib.vrt_volume_redo(r._ctx, EDITED, 1, C.byref(res)) == _abi.VRT_ERR_INVALID
        assert_same_buffers(buffers(r, EDITED), now, "after the refused redo")
        check_info(r, EDITED, hist, "after the refused redo")


def test_limits_entries_and_bytes():
    models, dabs = dab_models(n=3)
    with v.VHipRenderer(devices=(0,)) as r:
        upload_model(r, EDITED, models[0])
        hist = H.History(2, 1 << 40)
        r.enable_history(EDITED, 2, 1 << 40)
        for i, dab in enumerate(dabs):
            r.apply_brushes(EDITED, None, dab)
            hist.record(state_of(models[i]), state_of(models[i + 1]))
        assert hist.dropped == 1 and len(hist.undo) == 2
        check_info(r, EDITED, hist, "max_entries = 2: the third entry drops the first")
        r.undo(EDITED, 2)
        assert_same_buffers(buffers(r, EDITED), models[1].expected_buffers(), "the two entries left go back to after the first dab")
        assert r._lib.vrt_volume_undo(r._ctx, EDITED, 1, None) == _abi.VRT_ERR_INVALID
        # a limit in bytes between a dab and the whole grid: the dabs stay, the whole-grid redistance takes everything with it
        whole = models[3].copy()
        whole.redistance(3, 0)
        grid_tiles = len(H.changed_tiles(state_of(models[3]), state_of(whole)))
        dab_tiles = max(len(H.changed_tiles(state_of(a), state_of(b))) for a, b in zip(models, models[1:]))
        limit = 3 * dab_tiles * H.TILE_BYTES
        assert dab_tiles * H.TILE_BYTES <= limit < grid_tiles * H.TILE_BYTES, (dab_tiles, grid_tiles)
        upload_model(r, EDITED, models[0])
        hist.clear()
        hist.set_limits(100, limit)
        r.enable_history(EDITED, 100, limit)
        assert r.history_info(EDITED) == hist.info()  # the upload emptied the stacks; turning on again only set the limits: dropped stays 1
        for i, dab in enumerate(dabs):
            r.apply_brushes(EDITED, None, dab)
            hist.record(state_of(models[i]), state_of(models[i + 1]))
        assert len(hist.undo) == 3 and hist.dropped == 1
        check_info(r, EDITED, hist, "three dabs within the bytes")
        r.redistance(EDITED, None, 3, 0)
        hist.record(state_of(models[3]), state_of(whole))
        assert len(hist.undo) == 0 and hist.dropped == 5
        check_info(r, EDITED, hist, "the whole-grid entry exceeds max_bytes on its own")
        assert_same_buffers(buffers(r, EDITED), whole.expected_buffers(), "the redistance itself")
        r.apply_brushes(EDITED, None, dabs[0])  # and the history goes on
        after = whole.copy()
        after.brushes(dabs[0])
        hist.record(state_of(whole), state_of(after))
        check_info(r, EDITED, hist, "a dab after everything was dropped")
        r.undo(EDITED)
        assert_same_buffers(buffers(r, EDITED), whole.expected_buffers(), "undo of that dab")


def test_lifetime_upload_free_and_set_metric():
    models, dabs = dab_models(n=2)
    lib = _abi.load()
    with v.VHipRenderer(devices=(0,)) as r:
        upload_model(r, EDITED, models[0])
        r.enable_history(EDITED, 7, 1 << 30)
        hist = H.History(7, 1 << 30)
        r.apply_brushes(EDITED, None, dabs[0])
        hist.record(state_of(models[0]), state_of(models[1]))
        # set_metric between edit and undo: the stacks stay, and the undo rebuilds under the new metric
        _abi.check(lib.vrt_volume_set_metric(r._ctx, EDITED, 0.37, 31.0), "vrt_volume_set_metric")
        check_info(r, EDITED, hist, "after set_metric")
        r.undo(EDITED)
        restored = models[0].copy()
        restored.set_metric(0.37, 31.0)
        assert_same_buffers(buffers(r, EDITED), restored.expected_buffers(), "undo under the new metric")
        _abi.check(lib.vrt_volume_set_metric(r._ctx, EDITED, 1.0, 0.0), "vrt_volume_set_metric")  # ... and without the tables
        r.redo(EDITED)
        edited = models[1].copy()
        edited.set_metric(1.0, 0.0)
        assert_same_buffers(buffers(r, EDITED), edited.expected_buffers(), "redo without the tables")
        # an upload onto the slot empties the stacks and keeps the limits
        hist.undo_steps(state_of(models[1]))
        hist.redo_steps(state_of(models[0]))
        check_info(r, EDITED, hist, "before the upload")
        upload_model(r, EDITED, models[2])
        hist.clear()
        check_info(r, EDITED, hist, "after the upload")
        assert r.history_info(EDITED)["max_entries"] == 7 and lib.vrt_volume_undo(r._ctx, EDITED, 1, None) == _abi.VRT_ERR_INVALID
        # vrt_volume_free turns the history off
        _abi.check(lib.vrt_volume_free(r._ctx, EDITED), "vrt_volume_free")
        assert lib.vrt_volume_history_info(r._ctx, EDITED, C.byref(_abi.vrt_history_info())) == _abi.VRT_ERR_SLOT
        upload_model(r, EDITED, models[0])
        check_info(r, EDITED, None, "after free and upload: off")
        r.apply_brushes(EDITED, None, dabs[0])
        check_info(r, EDITED, None, "an edit with the history off records nothing")
        assert lib.vrt_volume_undo(r._ctx, EDITED, 1, None) == _abi.VRT_ERR_INVALID
        # turning it off frees everything; `dropped` starts again with the next turning on
        r.enable_history(EDITED, 1, 1 << 30)
        r.apply_brushes(EDITED, None, dabs[1])
        r.apply_brushes(EDITED, None, dabs[0])
        assert r.history_info(EDITED)["undo_entries"] == 1
        r.enable_history(EDITED, 0, 0)
        check_info(r, EDITED, None, "turned off")
        r.enable_history(EDITED, 3, 1 << 30)
        assert r.history_info(EDITED) == H.History(3, 1 << 30).info()


def test_refusals_change_nothing():
    models, dabs = dab_models(n=2)
    lib = _abi.load()
    info = _abi.vrt_history_info()
    res = _abi.vrt_brush_result()
    with v.VHipRenderer(devices=(0,)) as r:
        ctx = r._ctx
        upload_model(r, EDITED, models[0])
        r.enable_history(EDITED, 5, 1 << 30)
        r.apply_brushes(EDITED, None, dabs[0])
        r.apply_brushes(EDITED, None, dabs[1])
        r.undo(EDITED)
        held, held_info = buffers(r, EDITED), r.history_info(EDITED)
        assert (held_info["undo_entries"], held_info["redo_entries"]) == (1, 1)
        INV, SLOT = _abi.VRT_ERR_INVALID, _abi.VRT_ERR_SLOT
        refused = [
            (lib.vrt_volume_history(None, EDITED, 5, 1 << 30), INV), (lib.vrt_volume_history(ctx, EDITED, -1, 1 << 30), INV),
            (lib.vrt_volume_history(ctx, EDITED, 0, 1 << 30), INV), (lib.vrt_volume_history(ctx, EDITED, 5, 0), INV),
            (lib.vrt_volume_history(ctx, OTHER, 5, 1 << 30), SLOT), (lib.vrt_volume_history(ctx, _abi.VRT_MAX_VOLUMES, 5, 1 << 30), SLOT),
            (lib.vrt_volume_history_info(None, EDITED, C.byref(info)), INV), (lib.vrt_volume_history_info(ctx, EDITED, None), INV),
            (lib.vrt_volume_history_info(ctx, OTHER, C.byref(info)), SLOT),
            (lib.vrt_volume_undo(None, EDITED, 1, C.byref(res)), INV), (lib.vrt_volume_redo(None, EDITED, 1, C.byref(res)), INV),
            (lib.vrt_volume_undo(ctx, EDITED, 0, C.byref(res)), INV), (lib.vrt_volume_undo(ctx, EDITED, -3, C.byref(res)), INV),
            (lib.vrt_volume_undo(ctx, EDITED, 2, C.byref(res)), INV), (lib.vrt_volume_redo(ctx, EDITED, 0, C.byref(res)), INV),
            (lib.vrt_volume_redo(ctx, EDITED, 2, C.byref(res)), INV), (lib.vrt_volume_undo(ctx, OTHER, 1, C.byref(res)), SLOT),
            (lib.vrt_volume_redo(ctx, -1, 1, C.byref(res)), SLOT),
        ]
        for i, (got, want) in enumerate(refused):
            assert got == want, (i, got, want)
        assert_same_buffers(buffers(r, EDITED), held, "after the refused calls")
        assert r.history_info(EDITED) == held_info
        # a slot whose history is off refuses undo and redo
        upload_model(r, OTHER, models[0])
        r.apply_brushes(OTHER, None, dabs[0])
        other = buffers(r, OTHER)
        assert lib.vrt_volume_undo(ctx, OTHER, 1, C.byref(res)) == INV and lib.vrt_volume_redo(ctx, OTHER, 1, C.byref(res)) == INV
        assert_same_buffers(buffers(r, OTHER), other, "undo with the history off")
        # calls that change no bit record nothing and leave the redo stack alone
        N = models[0].N
        r.apply_brushes(EDITED, None, [v.sphere_brush(B.ADD, (-4.0 * N, 8.0, 8.0), 1.0, 0.0, 1.0, 2)])
        r.components(EDITED, _abi.components_record(CR.REPORT))
        box = r.download_region(EDITED, (2, 3, 4), (9, 9, 9))
        vol = v.VVoxelVolume(models[0].res, models[0].extent)
        vol.density, vol.material_id = np.zeros((N, N, N), np.float32), np.zeros((N, N, N), np.uint8)
        vol.density[2:10, 4:10, 3:10], vol.material_id[2:10, 4:10, 3:10] = box
        r.update_volume_region(EDITED, vol, (2, 3, 4), (9, 9, 9))  # F32: the bytes already held
        assert_same_buffers(buffers(r, EDITED), held, "after the calls that change nothing")
        assert r.history_info(EDITED) == held_info


# ---- a frame, and the adaptors -----------------------------------------------------------------------------------------------------------

def test_the_frame_after_edit_and_undo_is_the_frame_before():
    sc = scenes.config3_torus(5, 16)
    p = frame_params(sc)
    vol = sc.volumes()[0]
    vol.step_max = 0.5 * vol.GetCellSize()  # with the empty-space tables, so that the slot has an active box
    far = vol.N - 3.0
    with v.VHipRenderer(devices=(0,)) as r:
        set_frame(r, sc, p)
        first = r.Render()
        t_first = r.last_timing()
        r.enable_history(0, *BIG)
        box_before = buffers(r, 0)["active_box"]
        got = r.apply_brushes(0, None, [v.sphere_brush(B.ADD, (far, far, far), 2.5, 0.0, 2.0, 1)])  # a ball in the grid's corner, far from the torus
        assert got["written"] > 20 and not np.array_equal(buffers(r, 0)["active_box"], box_before), "the edit grew the active box"
        edited = r.Render()
        assert not same_bits(edited, first)
        assert r.undo(0)["written"] == got["written"]
        again = r.Render()
        t_again = r.last_timing()
        assert same_bits(again, first), f"{int((again.view(np.uint32) != first.view(np.uint32)).sum())} values differ"
        assert [t_again[k] for k in STAT_KEYS] == [t_first[k] for k in STAT_KEYS]
        r.redo(0)
        assert same_bits(r.Render(), edited)


def test_the_python_mirror_follows_undo_and_redo():
    models, dabs = dab_models(n=2)
    vol = v.VVoxelVolume(models[0].res, models[0].extent)
    vol.density, vol.material_id = np.array(models[0].stored), np.array(models[0].material)
    vol.density_scale, vol.step_max = models[0].scale, models[0].step
    with v.VHipRenderer(devices=(0,)) as r:
        r.upload_volume(EDITED, vol)
        r.enable_history(EDITED, *BIG)
        for dab in dabs:
            r.apply_brushes(EDITED, vol, dab)
        assert same_bits(vol.density, models[2].decoded())
        r.undo(EDITED, 2, vol)
        assert same_bits(vol.density, models[0].decoded()) and np.array_equal(vol.material_id, models[0].material)
        r.redo(EDITED, 1, vol)
        assert same_bits(vol.density, models[1].decoded()) and np.array_equal(vol.material_id, models[1].material)
        assert not vol.dirty and vol.dirty_box is None
        assert_same_buffers(buffers(r, EDITED), models[1].expected_buffers(), "the device beside the mirror")


def test_vrt_demo_undoes_its_dabs(tmp_path):
    """vrt_demo --undo K: six dabs on the device, all six undone in one call; the mesh that leaves equals the mesh of a run without edits."""
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    common = ["--frames", "6", "--size", "96x54"]
    outs = {}
    for name, extra in (("undone", ["--edit-device", "--edit-brush", "4", "--undo", "6"]), ("plain", []), ("edited", ["--edit-device", "--edit-brush", "4"])):
        os.mkdir(tmp_path / name)
        mesh = str(tmp_path / name / "mesh.glb")  # one file, and the same name in every run: the bytes can be compared
        run = subprocess.run([exe] + common + extra + ["--mesh-out", mesh, "--out", str(tmp_path / (name + ".ppm"))],
                             capture_output=True, text=True, timeout=180)
        assert run.returncode == 0, run.stdout + run.stderr
        outs[name] = (open(mesh, "rb").read(), run.stdout)
    lines = [l for l in outs["undone"][1].splitlines() if l.startswith("history:")]
    assert len(lines) == 2 and "undo_entries 6" in lines[0] and "undo_entries 0" in lines[1] and "redo_entries 6" in lines[1], lines
    assert outs["undone"][0] == outs["plain"][0] and outs["edited"][0] != outs["plain"][0]
