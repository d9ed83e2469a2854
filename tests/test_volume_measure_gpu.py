"""Volume measurement on the device (vrt_volume_measure) against the numpy reference of the contract (tests/measure_ref.py): tolerance 0
on every field and on all 256 material counts — the result is made of integers, so no schedule of waves and atomics may change it; the
host pass on the same voxels; that the call only reads the slot and leaves its history alone; a dab and its undo; the argument rules."""
import ctypes as C
import functools

import numpy as np
import pytest

import brush_ref as B
import fill_ref as F
import measure_ref as MS
import redistance_ref as RR
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx
from test_volume_fill_gpu import EDITED, FULL, assert_same_buffers, buffers, upload_field
from test_volume_measure import EXTENT, SIZES, Field, assert_same_result, boxes, case, cell_of, isos, reference

pytestmark = pytest.mark.gpu
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


def upload_case(r, f, slot=EDITED):
    vol = v.VVoxelVolume(f.resolution, f.extent).set_device_format(f.fmt)
    upload_field(r, slot, vol, f.fmt, f.stored, f.material)
    return vol


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", SIZES)
def test_device_measure_equals_the_reference(renderer, N, fmt):
    """5^3 (fewer cells than a wave), 9^3 and 17^3 with the planted values: every box, both levels; the slot's buffers untouched."""
    f = case(N, int(fmt))
    upload_case(renderer, f)
    before = buffers(renderer, EDITED)
    for box, (lo, hi) in boxes(N).items():
        for iso in isos(N):
            got = renderer.measure(EDITED, iso, lo, hi)
            assert_same_result(got, reference(N, int(fmt), iso, box), f"{N}^3, format {fmt}, iso {iso}, box {box}")
    assert_same_buffers(buffers(renderer, EDITED), before, f"{N}^3, format {fmt}")


@functools.lru_cache(maxsize=None)
def sphere(N):
    """An off-centre sphere on 33^3 / 65^3 (a row of 65 samples is two runs; the workgroups outnumber the device's at 65^3 and walk),
    with ids that differ from sample to sample; read-only."""
    d = RR.sphere_field(N, (0.47 * N, 0.55 * N, 0.43 * N), 0.29 * N, cell_of(N))
    m = F.hand_made_material(d)
    for a in (d, m):
        a.setflags(write=False)
    return d, m


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", (33, 65))
def test_spheres_over_many_workgroups(renderer, N, fmt):
    """The whole grid, and a box whose origin and size are odd on every axis and which cuts the sphere."""
    d, m = sphere(N)
    f = Field(d, int(fmt), m)
    upload_case(renderer, f)
    lo = (3, 5, 7)
    hi = tuple(l + s - 1 for l, s in zip(lo, (N - 12, N - 16, N - 10)))  # sizes N - 12, N - 16, N - 10: odd
    for box in ((None, None), (lo, hi)):
        want = MS.measure(f.stored, f.material, f.fmt, 0.0, *box)
        got = renderer.measure(EDITED, 0.0, *box)
        assert_same_result(got, want, f"sphere on {N}^3, format {fmt}, box {box}")
        assert want["active_cells"] > (400 if N == 33 else 2000) and want["subsamples"] > 64 * want["active_cells"]


def test_all_256_material_ids(renderer):
    d, _ = sphere(33)
    ids = (np.arange(d.size, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(d.shape)
    f = Field(np.full(d.shape, -1.0, np.float32), R.F32, ids)  # all INSIDE: every id counts
    upload_case(renderer, f)
    got, want = renderer.measure(EDITED), MS.measure(f.stored, f.material, f.fmt, 0.0)
    assert_same_result(got, want, "256 ids")
    assert min(want["material_samples"]) > 0 and sum(want["material_samples"]) == 33 ** 3
    g = Field(d, R.F32, ids)  # and on the sphere, where waves hold a mix of classes and of ids
    upload_case(renderer, g)
    assert_same_result(renderer.measure(EDITED), MS.measure(g.stored, g.material, g.fmt, 0.0), "256 ids on the sphere")


def raw_call(r, slot, iso=0.0, o=None, s=None, ctx=True, result=True, counts=True):
    res, cnt = _abi.vrt_measure_result(), (C.c_uint64 * 256)()
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    C.memset(cnt, 0xA5, C.sizeof(cnt))
    rc = r._lib.vrt_volume_measure(r._ctx if ctx else None, slot, iso, o, s, C.byref(res) if result else None, cnt if counts else None)
    return rc, bytes(res), bytes(cnt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_calls_return_the_same_bytes_and_the_host_pass_agrees(renderer, fmt):
    d, m = sphere(33)
    f = Field(d, int(fmt), m)
    upload_case(renderer, f)
    first, second = raw_call(renderer, EDITED), raw_call(renderer, EDITED)
    assert first[0] == _abi.VRT_OK and first == second
    res = _abi.vrt_measure_result.from_buffer_copy(first[1])
    assert tuple(res.reserved_) == (0, 0)
    host = vx.measure_host(f.host_volume(), 0.0, texel16=int(fmt) == R.TEXEL16)
    assert_same_result(renderer.measure(EDITED), host, f"device against host, format {fmt}")
    assert _abi.measure_dict(res, np.frombuffer(first[2], np.uint64)) == host
    # without the counts the record is the same
    rc, alone, untouched = raw_call(renderer, EDITED, counts=False)
    assert rc == _abi.VRT_OK and alone == first[1]


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_dab_changes_the_result_and_undo_brings_it_back(renderer, fmt):
    """With the history on: measuring records nothing and touches no buffer; a dab changes the result to the reference's of the edited
    volume; vrt_volume_undo brings the first result back."""
    d, m = sphere(33)
    f = Field(d, int(fmt), m)
    vol = upload_case(renderer, f)
    renderer.enable_history(EDITED, 8, 64 << 20)
    before, info = buffers(renderer, EDITED), renderer.history_info(EDITED)
    first = renderer.measure(EDITED)
    assert_same_result(first, MS.measure(f.stored, f.material, f.fmt, 0.0), "before the dab")
    assert_same_buffers(buffers(renderer, EDITED), before, "after measuring")
    assert renderer.history_info(EDITED) == info
    rec = v.sphere_brush(_abi.BRUSH_SUBTRACT, (24.6, 18.0, 14.0), 4.0, 1.5, 3.0, 0)
    want_d, want_m = np.array(f.stored), np.array(f.material)
    dab = renderer.apply_brushes(EDITED, None, [rec])
    assert dab == B.apply(want_d, want_m, f.fmt, [rec], vol.VolumeExtends, vol.density_scale) and dab["written"] > 50
    edited, info = renderer.measure(EDITED), renderer.history_info(EDITED)
    assert_same_result(edited, MS.measure(want_d, want_m, f.fmt, 0.0), "after the dab")
    assert edited["subsamples"] < first["subsamples"] and info["undo_entries"] == 1
    assert renderer.history_info(EDITED) == info
    renderer.undo(EDITED)
    assert_same_result(renderer.measure(EDITED), first, "after the undo")
    assert_same_buffers(buffers(renderer, EDITED), before, "after the undo")


def test_refused_calls_write_nothing(renderer):
    f = case(9, R.F32)
    upload_case(renderer, f)
    three = lambda *a: (C.c_int * 3)(*a)
    blank = (b"\xa5" * C.sizeof(_abi.vrt_measure_result), b"\xa5" * 2048)
    INVALID, SLOT = _abi.VRT_ERR_INVALID, _abi.VRT_ERR_SLOT
    for want, kw in ((INVALID, dict(ctx=False)), (INVALID, dict(result=False)), (INVALID, dict(iso=float("nan"))), (INVALID, dict(iso=float("-inf"))),
                     (INVALID, dict(o=three(0, 0, 0))), (INVALID, dict(s=three(2, 2, 2))), (INVALID, dict(o=three(0, 0, 0), s=three(2, 0, 2))),
                     (INVALID, dict(o=three(0, -1, 0), s=three(2, 2, 2))), (INVALID, dict(o=three(0, 0, 8), s=three(2, 2, 2))),
                     (SLOT, dict(slot=FULL)), (SLOT, dict(slot=-1)), (SLOT, dict(slot=_abi.VRT_MAX_VOLUMES))):
        rc, res, cnt = raw_call(renderer, kw.pop("slot", EDITED), **kw)
        assert rc == want and (res, cnt) == blank, (want, rc)
    rc, res, cnt = raw_call(renderer, EDITED, o=three(0, 0, 7), s=three(2, 2, 2))  # the last two planes: accepted
    assert rc == _abi.VRT_OK and res != blank[0]
