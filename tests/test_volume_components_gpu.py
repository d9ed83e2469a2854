"""Islands on the device (vrt_volume_components): after the call each device buffer of the slot — dense grid, materials, bricks, cell
records, both levels of the empty-space table, the Cube table and the active box — is byte-identical to the numpy reference of the
contract (tests/components_ref.py) pushed through the reference of the upload (tests/volume_ref.py), and to a full upload of that
field; result and list are the reference's; so frames and counters are those of the existing contract.  Tolerance 0 throughout."""
import ctypes as C
import functools

import numpy as np
import pytest

import components_ref as CR
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from test_volume_components import record_of
from test_volume_fill_gpu import EDITED, FULL, STAT_KEYS, assert_same_buffers, buffers, oracle_density, upload_field
from test_volume_fill_gpu import _fresh_slots  # noqa: F401 -- the autouse fixture: both slots start unused and are freed after

pytestmark = pytest.mark.gpu
FORMATS = [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16]
FIELDS = sorted(CR.hand_made_fields())
LIST_CAPACITY = 20


def hand_made_volume(fmt):
    vol = v.VVoxelVolume(5, 100.0)
    vol.step_max = 0.5 * vol.GetCellSize()  # both levels of the empty-space table live
    return vol.set_device_format(fmt)


@functools.lru_cache(maxsize=None)
def stored_field(name, fmt):
    d = CR.hand_made_fields()[name][0]
    stored, material = R.dense_field(d, fmt), CR.hand_made_material(d)
    stored.setflags(write=False), material.setflags(write=False)
    return stored, material


@functools.lru_cache(maxsize=None)
def reference(name, fmt, n):
    """The reference's answer to record n of the field (-1: REPORT), computed once and never written to afterwards."""
    stored, material = stored_field(name, fmt)
    kw = dict(op=CR.REPORT) if n < 0 else CR.hand_made_records()[name][n]
    want_d, want_m, info = CR.components(stored, material, fmt, list_capacity=LIST_CAPACITY, **kw)
    want_d.setflags(write=False), want_m.setflags(write=False)
    return kw, want_d, want_m, info


def call_and_check(r, vol, fmt, stored, material, kw, want_d, want_m, want, what):
    """Upload into EDITED, one call, result and list and every buffer against both witnesses; then a second call, which must write
    nothing (REMOVE_SEED: what the reference says of a second call)."""
    upload_field(r, EDITED, vol, fmt, stored, material)
    before = buffers(r, EDITED)
    got = r.components(EDITED, record_of(kw), None, LIST_CAPACITY)
    print(f"{what}: {({k: got[k] for k in got if k != 'list'})}")
    assert got == want, (what, got, want)
    have = buffers(r, EDITED)
    assert_same_buffers(have, R.device_bytes(want_d, want_m, fmt, vol.density_scale, vol.step_max), what + " against the reference")
    upload_field(r, FULL, vol, fmt, want_d, want_m)
    assert_same_buffers(have, buffers(r, FULL), what + " against a full upload")
    if want["written"] == 0:
        assert_same_buffers(have, before, what + ": nothing to remove, nothing changed")
    # a second call with the same record writes nothing — but REMOVE_SEED where the seed's neighbourhood holds a sample of another
    # component as well, which the seed then resolves to: the reference decides
    try:
        again_d, again_m, again_want = CR.components(want_d, want_m, fmt, list_capacity=LIST_CAPACITY, **kw)
    except CR.NoSolidSampleAtSeed:
        again_want = None
    assert kw["op"] == CR.REMOVE_SEED or (again_want is not None and again_want["written"] == 0), (what, again_want)
    if again_want is None:
        with pytest.raises(_abi.VrtError) as e:
            r.components(EDITED, record_of(kw), None, LIST_CAPACITY)
        assert e.value.status == _abi.VRT_ERR_INVALID, what
    else:
        assert r.components(EDITED, record_of(kw), None, LIST_CAPACITY) == again_want, what
        if again_want["written"]:
            have = buffers(r, EDITED)
            assert_same_buffers(have, R.device_bytes(again_d, again_m, fmt, vol.density_scale, vol.step_max), what + ", second call, against the reference")
    assert_same_buffers(buffers(r, EDITED), have, what + " after a second call")
    return got


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", FIELDS)
def test_hand_made_fields(renderer, name, fmt):
    stored, material = stored_field(name, fmt)
    vol = hand_made_volume(fmt)
    listed = CR.hand_made_fields()[name][1 if fmt == _abi.FORMAT_F32 else 2]
    for n in range(-1, len(CR.hand_made_records()[name])):
        kw, want_d, want_m, want = reference(name, fmt, n)
        if n < 0:  # the reference itself, and REPORT: every buffer as it was
            assert [(c["samples"], c["first"]) for c in want["list"]] == listed[:LIST_CAPACITY] and want["components"] == len(listed)
            assert want["written"] == 0
        call_and_check(renderer, vol, fmt, stored, material, kw, want_d, want_m, want, f"{name}, format {fmt}, {kw}")
    if name == "checkerboard":
        assert reference(name, fmt, 0)[3]["written"] == 33 ** 3 and reference(name, fmt, -1)[3]["components"] == 17969


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_seed_without_a_solid_sample_is_refused_after_the_read(renderer, fmt):
    stored, material = stored_field("ties", fmt)
    vol = hand_made_volume(fmt)
    upload_field(renderer, EDITED, vol, fmt, stored, material)
    before = buffers(renderer, EDITED)
    for op in (CR.REMOVE_SEED, CR.KEEP_SEED):
        with pytest.raises(_abi.VrtError) as e:
            renderer.components(EDITED, record_of(dict(op=op, gap=0.5, seed=CR.TIES_NO_SOLID_SEED)), None, 4)
        assert e.value.status == _abi.VRT_ERR_INVALID
    assert_same_buffers(buffers(renderer, EDITED), before, "after a seed that finds nothing")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["serpentine", "ties"])
def test_frame_after_the_call(renderer, name, fmt):
    """A frame of the edited slot and its counters equal those of a full upload of the reference's field."""
    kw, want_d, want_m, want = reference(name, fmt, 0)  # KEEP_LARGEST
    assert kw["op"] == CR.KEEP_LARGEST and want["removed"] == 1
    stored, material = stored_field(name, fmt)
    frames = {}
    for which, (d, m) in (("edited", (stored, material)), ("full", (want_d, want_m))):
        sc = scenes.config3_torus(5, 16)
        vol = sc.volumes()[0]
        vol.density, vol.material_id = oracle_density(d, fmt), np.array(m)
        vol.density_scale, vol.step_max = 20.0, 0.5 * vol.GetCellSize()
        vol.set_device_format(fmt)
        p = v.default_params(96, 54, scenes.min_cell(sc), 255, shadow=True)
        renderer.SetSceneToRender(sc)
        renderer.ResizeRenderOutput(p.width, p.height)
        renderer.params_override = p
        renderer.SetRendererMode(p.mode)
        renderer.Render()  # the scene's volume is resident in slot 0 now
        if fmt == _abi.FORMAT_TEXEL16:
            assert np.array_equal(buffers(renderer, 0)["dense"], np.ascontiguousarray(d).reshape(-1).view(np.uint8))
        if which == "edited":
            got = renderer.components(0, record_of(kw), vol, LIST_CAPACITY)
            assert got == want
            if fmt == _abi.FORMAT_F32:  # the mirror follows
                assert np.array_equal(vol.density.view(np.uint32), want_d.view(np.uint32)) and np.array_equal(vol.material_id, want_m)
        img = np.array(renderer.Render())
        t = renderer.last_timing()
        frames[which] = (img, {k: t[k] for k in STAT_KEYS}, buffers(renderer, 0))
    assert np.array_equal(frames["edited"][0], frames["full"][0]) and frames["edited"][1] == frames["full"][1]
    assert frames["full"][1]["hits"] > 0
    assert_same_buffers(frames["edited"][2], frames["full"][2], f"{name}, format {fmt}: the rendered slot against a full upload")


def test_refused_calls_change_nothing(renderer):
    fmt = _abi.FORMAT_TEXEL16
    stored, material = stored_field("ties", fmt)
    upload_field(renderer, EDITED, hand_made_volume(fmt), fmt, stored, material)
    before = buffers(renderer, EDITED)
    lib, ctx = renderer._lib, renderer._ctx
    res = _abi.vrt_components_result()
    lst = (_abi.vrt_component * 4)()
    good = dict(op=CR.REMOVE_SMALL, gap=0.5, min_samples=100)
    call = lambda ctx_, slot, kw, list_=lst, cap=4: lib.vrt_volume_components(ctx_, slot, C.byref(record_of(kw)) if kw else None, list_, cap, C.byref(res))
    assert call(ctx, 7, good) == _abi.VRT_ERR_SLOT
    assert call(ctx, _abi.VRT_MAX_VOLUMES, good) == _abi.VRT_ERR_SLOT
    assert call(ctx, -1, good) == _abi.VRT_ERR_SLOT
    assert call(None, EDITED, good) == _abi.VRT_ERR_INVALID
    assert call(ctx, EDITED, None) == _abi.VRT_ERR_INVALID
    bad = [dict(op=5), dict(op=-1), dict(material_id=256), dict(material_id=-2), dict(gap=float("nan")), dict(gap=float("inf")), dict(gap=0.0),
           dict(gap=-1.0), dict(gap=0.009), dict(op=CR.KEEP_LARGEST, min_samples=1), dict(op=CR.REPORT, min_samples=1), dict(seed=(0, 0, 1)),
           dict(op=CR.KEEP_SEED, min_samples=0, seed=(33, 0, 0)), dict(op=CR.REMOVE_SEED, min_samples=0, seed=(0, -1, 0)),
           dict(op=CR.REPORT, min_samples=0, gap=float("nan"))]
    for kw in bad:
        assert call(ctx, EDITED, dict(good, **kw)) == _abi.VRT_ERR_INVALID, kw
    reserved = record_of(good)
    reserved.reserved_[0] = 1
    assert lib.vrt_volume_components(ctx, EDITED, C.byref(reserved), lst, 4, C.byref(res)) == _abi.VRT_ERR_INVALID
    assert call(ctx, EDITED, good, lst, -1) == _abi.VRT_ERR_INVALID
    assert call(ctx, EDITED, good, None, 1) == _abi.VRT_ERR_INVALID
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")
    # REPORT ignores the gap, and neither a list nor a result record is needed
    report = record_of(dict(op=CR.REPORT, gap=-3.0))
    assert lib.vrt_volume_components(ctx, EDITED, C.byref(report), None, 0, None) == _abi.VRT_OK
    assert_same_buffers(buffers(renderer, EDITED), before, "after REPORT")


def test_a_context_over_two_devices_edits_both():
    fmt = _abi.FORMAT_TEXEL16
    kw, want_d, want_m, want = reference("serpentine", fmt, 0)
    stored, material = stored_field("serpentine", fmt)
    vol = hand_made_volume(fmt)
    with v.VHipRenderer(devices=(0, 0)) as r:
        upload_field(r, EDITED, vol, fmt, stored, material)
        got = r.components(EDITED, record_of(kw), None, LIST_CAPACITY)
        assert got == want
        ref = R.device_bytes(want_d, want_m, fmt, vol.density_scale, vol.step_max)
        for dev in (0, 1):
            assert_same_buffers(buffers(r, EDITED, dev), ref, f"device {dev} of two against the reference")
