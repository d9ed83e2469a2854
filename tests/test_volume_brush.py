"""CSG sculpt brushes (vrt_volume_apply_brushes / vrt_volume_download_region), the parts that need no GPU: argument checks without a
context, the ctypes layout of the two records, the numpy reference of the brush arithmetic (tests/brush_ref.py) checked against
direct expressions, and the new kernels' resources in the build's ISA listing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import brush_ref as B
import isa_listing
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRUSH_KERNELS = {"brush_region_kernel": "vrt_brush", "gather_region_kernel": "vrt_volume"}  # kernel: its listing


def test_brush_entry_points_refuse_a_null_context_without_a_gpu():
    lib = _abi.load()
    rec = (_abi.vrt_brush * 1)(v.sphere_brush(_abi.BRUSH_ADD, (1, 1, 1), 1.0))
    res = _abi.vrt_brush_result()
    assert lib.vrt_volume_apply_brushes(None, 0, 1, rec, C.byref(res)) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_apply_brushes(None, 0, 0, None, None) == _abi.VRT_ERR_INVALID
    o, s = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(1, 1, 1)
    out = np.zeros(8, np.uint8)
    assert lib.vrt_volume_download_region(None, 0, o, s, out.ctypes.data_as(C.c_void_p)) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_download_region(None, 0, o, s, None) == _abi.VRT_ERR_INVALID


def test_brush_records_have_the_c_layout(tmp_path):
    fields = ("shape", "op", "a", "b", "radius", "blend", "reach", "material", "reserved_")
    rfields = ("lo", "hi", "written")
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\nint main(void){\n'
        'printf("%zu %zu %d", sizeof(vrt_brush), sizeof(vrt_brush_result), VRT_MAX_BRUSHES);\n'
        + "".join(f'printf(" %zu", offsetof(vrt_brush, {f}));\n' for f in fields)
        + "".join(f'printf(" %zu", offsetof(vrt_brush_result, {f}));\n' for f in rfields)
        + 'printf(" %d %d %d %d %d %d\\n", VRT_BRUSH_SPHERE, VRT_BRUSH_BOX, VRT_BRUSH_CAPSULE, VRT_BRUSH_ADD, VRT_BRUSH_SUBTRACT,'
        " VRT_BRUSH_PAINT);\nreturn 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_abi.vrt_brush), C.sizeof(_abi.vrt_brush_result), _abi.MAX_BRUSHES]
    want += [getattr(_abi.vrt_brush, f).offset for f in fields] + [getattr(_abi.vrt_brush_result, f).offset for f in rfields]
    want += [_abi.BRUSH_SPHERE, _abi.BRUSH_BOX, _abi.BRUSH_CAPSULE, _abi.BRUSH_ADD, _abi.BRUSH_SUBTRACT, _abi.BRUSH_PAINT]
    assert got == want
    assert got[:3] == [64, 32, 32]
    assert (B.SPHERE, B.BOX, B.CAPSULE, B.ADD, B.SUBTRACT, B.PAINT) == tuple(want[-6:])


def analytic(res=5, extent=100.0):
    """A true SDF sampled on the grid: the torus the GPU tests use."""
    vol = v.torus_volume(res, extent, 55.0, 22.0)
    return vol, np.array(vol.density, np.float32), (vol.density <= 0).astype(np.uint8)


def test_reference_hard_sphere_equals_the_direct_expression():
    vol, dense, mat = analytic()
    n = vol.N
    cell, unit = B.units(n, vol.VolumeExtends, 1.0)
    assert cell == np.float32(vol.GetCellSize()) and unit == cell
    i = np.arange(n, dtype=np.float32)
    x, z, y = i[:, None, None], i[None, :, None], i[None, None, :]
    c, r = (20, 9, 14), np.float32(5.0)
    direct = ((np.sqrt(((x - c[0]) ** 2 + (y - c[1]) ** 2) + (z - c[2]) ** 2) - r) * cell).astype(np.float32)
    for op, merged in ((B.ADD, np.minimum(dense, direct)), (B.SUBTRACT, np.maximum(dense, -direct))):
        got_d, got_m = dense.copy(), mat.copy()
        rec = v.sphere_brush(op, c, float(r), reach=float(4 * n), material=3)  # the reach covers the grid: every sample is looked at
        res = B.apply(got_d, got_m, R.F32, [rec], vol.VolumeExtends, 1.0)
        assert np.array_equal(got_d, merged.astype(np.float32))
        changed = merged != dense
        assert res["written"] == int(changed.sum()) > 0
        assert np.array_equal(got_m[changed], np.where(merged[changed] <= 0, 3, 0)) and np.array_equal(got_m[~changed], mat[~changed])
        xs, zs, ys = np.nonzero(changed)
        assert res["lo"] == (xs.min(), ys.min(), zs.min()) and res["hi"] == (xs.max(), ys.max(), zs.max())


def test_reference_box_and_capsule_distances():
    n = 17
    box = v.box_brush(_abi.BRUSH_ADD, (8, 8, 8), (3, 2, 4))
    s = B.brush_distance(box, n)  # [x, z, y]
    assert s[8, 8, 8] == -2.0 and s[11, 8, 8] == 0.0 and s[13, 8, 8] == 2.0 and s[8, 8, 11] == 1.0 and s[8, 13, 8] == 1.0
    assert s[12, 13, 11] == np.float32(np.sqrt(np.float32(3.0)))  # one cell out on every axis: a corner
    rounded = v.box_brush(_abi.BRUSH_ADD, (8, 8, 8), (3, 3, 3), rounding=1.0)
    s = B.brush_distance(rounded, n)
    assert s[11, 8, 8] == 0.0 and s[8, 8, 8] == -3.0
    assert s[11, 11, 11] == np.float32(np.sqrt(np.float32(3.0)) - np.float32(1.0))  # the rounded corner lies inside the sharp one
    cap = v.capsule_brush(_abi.BRUSH_ADD, (4, 8, 8), (12, 8, 8), 2.0)
    s = B.brush_distance(cap, n)
    assert s[8, 8, 8] == -2.0 and s[8, 8, 11] == 1.0 and s[1, 8, 8] == 1.0 and s[15, 8, 8] == 1.0 and s[4, 11, 12] == 3.0
    assert B.brush_distance(v.sphere_brush(_abi.BRUSH_ADD, (2.5, 3, 4), 1.5), n)[3, 4, 3] == -1.0


def records():
    return [v.sphere_brush(_abi.BRUSH_SUBTRACT, (25, 16, 20), 5.0, reach=2.0, material=0),
            v.sphere_brush(_abi.BRUSH_ADD, (16.4, 25.2, 20), 4.0, blend=2.0, reach=6.0, material=2),
            v.capsule_brush(_abi.BRUSH_SUBTRACT, (10, 14.5, 12), (24, 20, 22), 2.5, blend=1.5, reach=3.0, material=0),
            v.box_brush(_abi.BRUSH_ADD, (16, 8, 16), (5, 2, 3), rounding=1.0, reach=4.0, material=-1),
            v.sphere_brush(_abi.BRUSH_PAINT, (16, 8, 16), 6.0, material=9)]


@pytest.mark.parametrize("fmt", [R.F32, R.TEXEL16])
def test_reference_n_records_equal_n_applications(fmt):
    vol, dense, mat = analytic()
    stored = R.dense_field(dense, fmt)
    one_d, one_m = stored.copy(), mat.copy()
    res = B.apply(one_d, one_m, fmt, records(), vol.VolumeExtends, 1.0)
    seq_d, seq_m = stored.copy(), mat.copy()
    union = np.zeros(stored.shape, bool)
    for rec in records():
        before_d, before_m = seq_d.copy(), seq_m.copy()
        step = B.apply(seq_d, seq_m, fmt, [rec], vol.VolumeExtends, 1.0)
        assert step["written"] > 0
        union |= (before_d.view(np.uint32) != seq_d.view(np.uint32)) | (before_m != seq_m)
    assert np.array_equal(one_d.view(np.uint32), seq_d.view(np.uint32)) and np.array_equal(one_m, seq_m)
    assert res["written"] >= int(union.sum()) > 1000  # a sample written back to its old bits still counts as written
    assert (one_m == 9).any() and (one_m == 2).any()


def test_reference_keeps_the_texels_it_does_not_write():
    """8088 of the 32768 texel values do not survive decode + encode; a brush whose comparison fails everywhere moves none."""
    q = np.arange(32768, dtype=np.float32)
    back = R.texel16_field((q * np.float32(0.01)).astype(np.float32))
    assert int((back != q).sum()) == 8088 and [int(x) for x in q[back != q][:5]] == [5, 10, 15, 20, 23]
    vol = v.torus_volume(6, 100.0, 55.0, 22.0)
    stored = R.texel16_field(np.array(vol.density, np.float32))
    mat = (vol.density <= 0).astype(np.uint8)
    rec = v.sphere_brush(_abi.BRUSH_SUBTRACT, (32, 32, 32), 2.0, reach=20.0, material=0)
    foot = B.brush_distance(rec, vol.N) < np.float32(20.0)
    fragile = R.texel16_field(B.decode(stored, R.TEXEL16)) != stored
    assert int(foot.sum()) == 44395 and int((foot & (vol.density <= 0)).sum()) == 13780 and int((foot & fragile).sum()) == 10068
    got_d, got_m = stored.copy(), mat.copy()
    res = B.apply(got_d, got_m, R.TEXEL16, [rec], vol.VolumeExtends, 1.0)
    assert res == {"written": 0, "lo": (65, 65, 65), "hi": (-1, -1, -1)}
    assert np.array_equal(got_d.view(np.uint32), stored.view(np.uint32)) and np.array_equal(got_m, mat)


def test_reference_figures_of_the_carved_torus():
    vol = v.torus_volume(6, 100.0, 55.0, 22.0)
    dense = np.array(vol.density, np.float32)
    mat = (dense <= 0).astype(np.uint8)
    recs = [v.sphere_brush(_abi.BRUSH_SUBTRACT, (50, 32, 40), 5.0, reach=2.0, material=0),
            v.sphere_brush(_abi.BRUSH_ADD, (32, 50, 40), 4.0, blend=2.0, reach=6.0, material=1),
            v.capsule_brush(_abi.BRUSH_SUBTRACT, (24, 30, 28), (40, 34, 36), 3.0, blend=1.5, reach=2.0, material=0)]
    got_d, got_m = dense.copy(), mat.copy()
    res = B.apply(got_d, got_m, R.F32, recs, vol.VolumeExtends, 1.0)
    assert res["written"] > 1000 and int((got_m != mat).sum()) > 100  # non-trivial footprints
    assert all(l <= h for l, h in zip(res["lo"], res["hi"]))
    nan = dense.copy()
    nan[40:60, 30:50, 25:40] = np.nan  # NaN densities are never written
    keep = nan.copy()
    B.apply(nan, mat.copy(), R.F32, recs, vol.VolumeExtends, 1.0)
    assert np.array_equal(np.isnan(nan), np.isnan(keep))


def test_brush_kernels_use_no_scratch_memory():
    found = {k: isa_listing.instances(isa_listing.kernels(stem), k) for k, stem in BRUSH_KERNELS.items()}
    assert all(found.values()), found
    assert len(found["brush_region_kernel"]) == 2  # F32 and TEXEL16
    for inst in found.values():
        for name, r in inst.items():
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["group_segment_fixed_size"] == 0, (name, r)
