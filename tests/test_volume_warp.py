"""vrt_volume_warp on the host (VVolumeConverter::Warp through libvrt_host.so's vrh_warp, which compiles the same csrc/warp_core.h as
the HIP kernels) against the numpy reference of the contract (tests/warp_ref.py): tolerance 0 on density bits, material bytes and the
result record.  Also the argument rules, which need no GPU, the ctypes layout of the record, and the properties of the rule — each
asserted on the reference first, so that a vacuous case fails here and not on the device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import brush_ref as B
import volume_ref as R
import volumetricraytracer_amd as v
import warp_cases as K
import warp_ref as W
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])

# What the rule is worth (include/vrt.h): (RMS, mean) of the crossings' radial error in cells, measured with
# warp_ref.worth and written into the header.
HEADER_WORTH = {"grab by (2.3, -1.1, 0.7)": (0.0270, -0.0266), "grab by (0.5, 0.5, 0.5)": (0.0370, -0.0367),
                "scale by 1.25": (0.0305, -0.0292), "inflate by 1.5": (0.0049, -0.0038)}


def host_warp(stored, material, fmt, rec):
    """vrh_warp on the stored field itself: (stored', material', result)."""
    N = stored.shape[0]
    voxels = np.zeros(stored.size, VOXEL)
    voxels["density"], voxels["material"] = stored.reshape(-1), material.reshape(-1)
    res = _abi.vrt_brush_result()
    rc = vx.load_host().vrh_warp(voxels.ctypes.data, N, (N - 1) / 2.0, 1.0, int(fmt == R.TEXEL16), C.byref(rec), C.byref(res))
    assert rc == _abi.VRT_OK
    shape = (N, N, N)
    return (np.ascontiguousarray(voxels["density"]).reshape(shape), np.ascontiguousarray(voxels["material"]).reshape(shape),
            {"written": int(res.written), "lo": tuple(res.lo), "hi": tuple(res.hi)})


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check(what, stored, material, fmt, rec, want):
    want_d, want_m, info = want[:3]
    got_d, got_m, got = host_warp(stored, material, fmt, rec)
    assert got["written"] == info["written"], (what, got, info)
    if info["written"]:
        assert got == info, (what, got, info)
    else:
        assert all(l > h for l, h in zip(got["lo"], got["hi"])), (what, got)
    assert same_bits(got_d, want_d), what
    assert np.array_equal(got_m, want_m), what
    return info


@pytest.mark.parametrize("fmt", K.FORMATS)
@pytest.mark.parametrize("N", K.SIZES)
def test_host_warp_equals_the_reference_over_the_sweep(N, fmt):
    stored, material = K.field(N, fmt)
    for what, rec in K.sweep(N):
        info = check(f"{what} ({N}^3, format {fmt})", stored, material, fmt, rec, K.sweep_reference(N, fmt, rec))
        assert info["written"] > 0, (what, N, fmt)  # the sweep is not vacuous anywhere


@pytest.mark.parametrize("fmt", K.FORMATS)
@pytest.mark.parametrize("N", K.SMALL)
def test_host_warp_on_the_smallest_grids(N, fmt):
    """Resolutions 0, 1, 2 over a field with NaN and +-0 samples: the cell clamp to N - 2 is the whole story."""
    stored, material = K.small_field(N, fmt)
    written = 0
    for what, rec in K.small_cases(N):
        written += check(f"{what} ({N}^3, format {fmt})", stored, material, fmt, rec, K.reference(stored, material, fmt, rec, ("small", N)))["written"]
    assert written > 0


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_an_identity_motion_writes_nothing(fmt):
    """Rule 5.  On a TEXEL16 slot decode + encode alone would move q = 5, 10, 15, ... down by one: the field holds such texels."""
    N = 17
    stored, material = K.field(N, fmt)
    if fmt == R.TEXEL16:
        q = np.abs(stored)
        assert int(((q == 5) | (q == 10) | (q == 15) | (q == 20) | (q == 23)).sum()) > 0
    for rec in K.identity_cases(N):
        want = W.warp(stored, material, fmt, rec)
        assert want[2]["written"] == 0 and want[3] == 0
        assert int(W.weights(rec, N)[0].sum()) == N ** 3  # every sample is in the region
        check(f"identity, material {rec.material}, format {fmt}", stored, material, fmt, rec, want)


def test_an_integer_grab_is_a_copy():
    stored, material, rec = K.copy_case()
    N = stored.shape[0]
    want = W.warp(stored, material, R.F32, rec)
    check("integer grab", stored, material, R.F32, rec, want)
    gx, gy, gz = K.COPY_GRAB
    full = B.brush_distance(rec, N) <= np.float32(-rec.falloff)
    x, z, y = np.nonzero(full)
    assert x.size > 5000
    assert x.min() - gx >= 0 and z.min() - gz >= 0 and y.min() - gy >= 0 and max(x.max() - gx, z.max() - gz, y.max() - gy) < N
    for got in (want[0], host_warp(stored, material, R.F32, rec)[0]):
        assert np.array_equal(got[x, z, y].view(np.uint32), stored[x - gx, z - gz, y - gy].view(np.uint32))
    assert np.array_equal(want[1][x, z, y], material[x - gx, z - gz, y - gy])  # ... and with SOURCE, its id


def test_jacobi_matters():
    """The 65^3 case tells the rule from an in-place pass: at least 1000 samples differ."""
    stored, material, rec = K.jacobi_case(R.F32)
    want = W.warp(stored, material, R.F32, rec)
    in_place_d, in_place_m = W.warp_in_place(stored, material, R.F32, rec)
    differ = int((in_place_d.view(np.uint32) != want[0].view(np.uint32)).sum())
    print("in place differs from the rule in", differ, "densities and", int((in_place_m != want[1]).sum()), "ids")
    assert differ >= 1000
    info = want[2]
    spans = [h - l + 1 for l, h in zip(info["lo"], info["hi"])]
    assert all(s >= 38 for s in spans) and all(l % 4 != 0 and l > 8 for l in info["lo"]) and all(h < 65 - 9 for h in info["hi"]), info
    check("Jacobi, 65^3", stored, material, R.F32, rec, want)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_a_source_beyond_the_grid_is_the_face(fmt):
    stored, material, rec = K.clamp_case(fmt)
    N = stored.shape[0]
    G = W.geometry(rec, N, np.float32(1.0))
    assert int((G["region"] & (G["r"][2] < 0)).sum()) >= 100
    want = W.warp(stored, material, fmt, rec)
    assert want[2]["written"] > 100 and want[2]["lo"][2] == 0
    check(f"clamp at z = 0, format {fmt}", stored, material, fmt, rec, want)


def test_material_only_writes():
    stored, material, rec = K.material_only_case()
    want = W.warp(stored, material, R.F32, rec)
    assert want[3] == 0 and want[2]["written"] > 100
    assert same_bits(want[0], stored)
    check("material only", stored, material, R.F32, rec, want)


def test_nan_is_never_stored():
    N = 17
    stored = np.array(K.field(N, R.F32)[0])
    c = (N - 1) // 2
    stored[c + 4, c, c] = np.float32(np.nan)
    material = np.zeros((N, N, N), np.uint8)
    rec = v.warp_record(_abi.BRUSH_SPHERE, (c + 5.0, c, c), (0, 0, 0), 5.5, pull=K.grab((1.5, 0.5, -0.5)), falloff=1.0, material=2)
    want = W.warp(stored, material, R.F32, rec)
    check("a NaN among the taps", stored, material, R.F32, rec, want)
    assert not np.isnan(want[0][~np.isnan(stored)]).any() and want[2]["written"] > 100  # no NaN is stored where there was none
    kept = W.weights(rec, N)[0] & (want[0].view(np.uint32) == stored.view(np.uint32))
    assert int(kept.sum()) >= 4  # the samples whose taps hold the NaN keep their bits


def test_everything_outside_the_region_keeps_its_bits():
    N = 33
    for fmt in K.FORMATS:
        stored, material = K.field(N, fmt)
        for shape in K.SHAPES:
            rec = v.warp_record(pull=K.grab((1.5, 0.0, -2.5)), falloff=1.0, material=9, **K.region_of(N, shape))
            got_d, got_m, got = host_warp(stored, material, fmt, rec)
            region = W.weights(rec, N)[0]
            assert 0 < got["written"] <= int(region.sum()) < N ** 3
            assert np.array_equal(got_d.view(np.uint32)[~region], stored.view(np.uint32)[~region])
            assert np.array_equal(got_m[~region], material[~region])


def test_a_region_wholly_outside_the_grid_writes_nothing():
    N = 9
    stored, material = K.field(N, R.F32)
    for region in (dict(shape=_abi.BRUSH_SPHERE, a=(-20.0, 4.0, 4.0), b=(0, 0, 0), radius=3.0),
                   dict(shape=_abi.BRUSH_BOX, a=(4.0, 4.0, 40.0), b=(2.0, 2.0, 2.0), radius=0.0),
                   dict(shape=_abi.BRUSH_CAPSULE, a=(4.0, -9.0, 4.0), b=(30.0, -9.0, 4.0), radius=2.0)):
        rec = v.warp_record(pull=K.grab((1.0, 1.0, 1.0)), **region)
        got_d, got_m, got = host_warp(stored, material, R.F32, rec)
        assert got["written"] == 0 and all(l > h for l, h in zip(got["lo"], got["hi"])), got
        assert same_bits(got_d, stored) and np.array_equal(got_m, material)
        assert W.warp(stored, material, R.F32, rec)[2]["written"] == 0


def test_inflate_is_in_cells_of_the_volume():
    """off = inflate * unit: a volume whose cell is not 1 and whose density unit is not a cell."""
    N = 17
    stored, material = K.field(N, R.F32)
    rec = v.warp_record(inflate=1.5, falloff=2.0, material=4, **K.region_of(N, _abi.BRUSH_SPHERE))
    want = W.warp(stored, material, R.F32, rec, extent=20.0, density_scale=3.0)
    voxels = np.zeros(stored.size, VOXEL)
    voxels["density"], voxels["material"] = stored.reshape(-1), material.reshape(-1)
    res = _abi.vrt_brush_result()
    assert vx.load_host().vrh_warp(voxels.ctypes.data, N, 20.0, 3.0, 0, C.byref(rec), C.byref(res)) == _abi.VRT_OK
    assert int(res.written) == want[2]["written"] > 0
    assert same_bits(voxels["density"].reshape(N, N, N), want[0]) and not same_bits(want[0], W.warp(stored, material, R.F32, rec)[0])


def test_what_the_rule_is_worth():
    """A regression pin on the reference, not on the code under test: the header's four figures, recomputed."""
    got = W.worth(v.warp_record)
    for name, (rms, mean) in got.items():
        print(f"{name}: rms {rms:.4f} mean {mean:+.4f}")
    assert set(got) == set(HEADER_WORTH)
    for name, (rms, mean) in got.items():
        want_rms, want_mean = HEADER_WORTH[name]
        assert rms <= want_rms * 1.1 and abs(mean) <= abs(want_mean) * 1.1, (name, rms, mean)


def test_warp_from_motion_is_the_inverse_motion():
    pivot, shift, k = np.array([7.5, 3.25, 9.0]), np.array([1.0, -2.0, 0.5]), 1.6
    q = v.quat_from_axis_angle((0.3, -0.5, 0.8), 0.7)
    pull, length_scale = v.warp_from_motion(pivot, shift, q, k)
    assert length_scale == k and pull.shape == (3, 4)
    p = np.array([4.0, 11.0, -2.0])
    moved = pivot + k * np.array(v.quat_rotate(q, tuple(p - pivot)), np.float64) + shift
    assert np.allclose(pull[:, :3] @ moved + pull[:, 3], p, atol=1e-5)
    assert np.array_equal(v.warp_from_motion((1.0, 2.0, 3.0))[0], np.array(W.IDENTITY).reshape(3, 4))
    with pytest.raises(ValueError):
        v.warp_from_motion(pivot, rotation=(0, 0, 0, 0))
    with pytest.raises(ValueError):
        v.warp_from_motion(pivot, scale=0.0)


def good_record():
    return v.warp_record(_abi.BRUSH_SPHERE, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 2.0, pull=K.grab((0.5, 0.0, 0.25)), strength=0.5, falloff=1.0, material=3)


def refused_records():
    """[(what, record)]: one per VRT_ERR_INVALID rule of vrt.h that the record itself can break."""
    out = []

    def bad(what, **fields):
        r = good_record()
        for k, val in fields.items():
            if k in ("a0", "a1", "a2", "b0", "b1", "b2"):
                getattr(r, k[0])[int(k[1])] = val
            elif k.startswith("pull"):
                r.pull[int(k[4:])] = val
            elif k == "reserved":
                r.reserved_[val] = 1
            else:
                setattr(r, k, val)
        out.append((what, r))

    bad("unknown shape", shape=3)
    bad("negative shape", shape=-1)
    for name in ("radius", "strength", "falloff", "length_scale", "inflate", "a0", "a2", "b1", "pull0", "pull7", "pull11"):
        for val in (math.nan, math.inf, -math.inf):
            bad(f"{name} {val}", **{name: val})
    bad("strength 0", strength=0.0)
    bad("strength < 0", strength=-0.5)
    bad("strength > 1", strength=1.0001)
    bad("falloff 0", falloff=0.0)
    bad("falloff < 0", falloff=-1.0)
    bad("length_scale 0", length_scale=0.0)
    bad("length_scale < 0", length_scale=-1.0)
    bad("sphere radius 0", radius=0.0)
    bad("sphere radius < 0", radius=-1.0)
    bad("capsule radius 0", shape=_abi.BRUSH_CAPSULE, b0=5.0, radius=0.0)
    bad("capsule with a == b", shape=_abi.BRUSH_CAPSULE, b0=1.0, b1=1.0, b2=1.0)
    bad("box half size 0", shape=_abi.BRUSH_BOX, b0=0.0, b1=1.0, b2=1.0)
    bad("box half size < 0", shape=_abi.BRUSH_BOX, b0=1.0, b1=1.0, b2=-1.0)
    bad("box rounding < 0", shape=_abi.BRUSH_BOX, b0=1.0, b1=1.0, b2=1.0, radius=-0.5)
    bad("material 256", material=256)
    bad("material -3", material=-3)
    for w in range(7):
        bad(f"reserved word {w}", reserved=w)
    return out


def accepted_records():
    out = []
    singular = dict(pull0=0.0, pull5=0.0, pull10=0.0)
    for name, fields in (("strength exactly 1", dict(strength=1.0)), ("a tiny strength", dict(strength=1e-30)),
                         ("material -1", dict(material=-1)), ("material -2", dict(material=-2)), ("material 0", dict(material=0)),
                         ("material 255", dict(material=255)), ("a box without rounding", dict(shape=_abi.BRUSH_BOX, radius=0.0)),
                         ("a capsule", dict(shape=_abi.BRUSH_CAPSULE)), ("a huge falloff", dict(falloff=1e30)),
                         ("a zero matrix", singular), ("a negative inflate", dict(inflate=-3.0)), ("a tiny length_scale", dict(length_scale=1e-30)),
                         ("a huge translation", dict(pull3=1e30))):
        r = good_record()
        r.b[0], r.b[1], r.b[2] = 2.0, 1.0, 1.5  # half sizes of the box, the capsule's second end; a sphere ignores it
        for k, val in fields.items():
            if k.startswith("pull"):
                r.pull[int(k[4:])] = val
            else:
                setattr(r, k, val)
        out.append((name, r))
    return out


def test_argument_rules_without_a_gpu():
    """Through the C-ABI a NULL context or record is refused before anything else; every rule a record can break is checked by
    vrt_warp_core::valid, which vrt_volume_warp calls before it looks at the slot and which vrh_warp reaches without a context (the
    same rules on a live context, and VRT_ERR_SLOT: tests/test_volume_warp_gpu.py)."""
    lib = _abi.load()
    res = _abi.vrt_brush_result()
    good = good_record()
    assert lib.vrt_volume_warp(None, 0, C.byref(good), C.byref(res)) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_warp(None, 0, None, None) == _abi.VRT_ERR_INVALID
    host = vx.load_host()
    d = np.zeros(27, VOXEL)
    call = lambda rec, voxels=d, n=3: host.vrh_warp(voxels.ctypes.data if voxels is not None else None, n, 1.0, 1.0, 0, rec, C.byref(res))
    assert call(C.byref(good)) == _abi.VRT_OK
    assert call(None) == _abi.VRT_ERR_INVALID
    assert call(C.byref(good), voxels=None) == _abi.VRT_ERR_INVALID and call(C.byref(good), n=1) == _abi.VRT_ERR_INVALID
    for what, rec in refused_records():
        assert call(C.byref(rec)) == _abi.VRT_ERR_INVALID, what
    for what, rec in accepted_records():
        assert call(C.byref(rec)) == _abi.VRT_OK, what


def test_warp_record_has_the_c_layout(tmp_path):
    fields = ("shape", "material", "a", "b", "radius", "strength", "falloff", "pull", "length_scale", "inflate", "reserved_")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\nint main(void){\nprintf("%zu", sizeof(vrt_warp));\n'
                    + "".join(f'printf(" %zu", offsetof(vrt_warp, {f}));\n' for f in fields)
                    + 'printf(" %d %d\\n", VRT_WARP_MATERIAL_KEEP, VRT_WARP_MATERIAL_SOURCE);\nreturn 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_abi.vrt_warp)] + [getattr(_abi.vrt_warp, f).offset for f in fields] + [_abi.WARP_MATERIAL_KEEP, _abi.WARP_MATERIAL_SOURCE]
    assert got == want and got[0] == 128
    assert "vrt_volume_warp" in _abi.SYMBOLS


def test_warp_host_on_a_volume():
    """voxelizer.warp_host, the adaptor around vrh_warp: the volume follows in place and is marked dirty."""
    N = 17
    stored, material = K.field(N, R.F32)
    vol = K.volume(N)
    vol.density, vol.material_id = np.array(stored), np.array(material)
    what, rec = K.sweep(N)[1]
    want_d, want_m, info, _ = K.sweep_reference(N, R.F32, rec)
    assert vx.warp_host(vol, rec) == info and info["written"] > 0 and vol.dirty
    assert same_bits(vol.density, want_d) and np.array_equal(vol.material_id, want_m)
    bad = good_record()
    bad.strength = 0.0
    with pytest.raises(_abi.VrtError):
        vx.warp_host(vol, bad)
