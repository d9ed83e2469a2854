"""vrt_volume_stamp on the host (VVolumeConverter::Stamp through libvrt_host.so's vrh_stamp, which compiles the same csrc/stamp_core.h
as the HIP kernel) against the numpy reference of the contract (tests/stamp_ref.py): tolerance 0 on density bits, material bytes and
the result record.  Also the argument rules, which need no GPU, and the ctypes layout of the record."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import stamp_cases as K
import stamp_ref as S
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])


def records_of(stored, material):
    rec = np.zeros(stored.size, VOXEL)
    rec["density"], rec["material"] = stored.reshape(-1), material.reshape(-1)
    return rec


def host_stamp(src_kind, dst_kind, Nd, Ns, dfmt, sfmt, rec):
    """vrh_stamp on the stored fields themselves: (stored, material, result) of the destination afterwards, and the source's records
    before and after."""
    dst, src = K.volume(dst_kind, Nd, "dst"), K.volume(src_kind, Ns, "src")
    d = records_of(K.stored(dst_kind, Nd, "dst", dfmt), dst.material_id)
    s = records_of(K.stored(src_kind, Ns, "src", sfmt), src.material_id)
    s_before = s.copy()
    res = _abi.vrt_brush_result()
    rc = vx.load_host().vrh_stamp(d.ctypes.data, Nd, float(dst.VolumeExtends), float(dst.density_scale), int(dfmt == R.TEXEL16), s.ctypes.data, Ns,
                                  float(src.VolumeExtends), float(src.density_scale), int(sfmt == R.TEXEL16), C.byref(rec), C.byref(res))
    assert rc == _abi.VRT_OK
    assert s.tobytes() == s_before.tobytes()  # the source is only read
    shape = (Nd, Nd, Nd)
    return (np.ascontiguousarray(d["density"]).reshape(shape), np.ascontiguousarray(d["material"]).reshape(shape),
            {"written": int(res.written), "lo": tuple(res.lo), "hi": tuple(res.hi)})


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check(case, Nd, Ns, dfmt, sfmt):
    what, src_kind, dst_kind, rec = case
    want_d, want_m, want = K.reference(src_kind, dst_kind, Nd, Ns, dfmt, sfmt, rec)
    got_d, got_m, got = host_stamp(src_kind, dst_kind, Nd, Ns, dfmt, sfmt, rec)
    what = f"{what} ({Ns}^3 fmt {sfmt} into {Nd}^3 fmt {dfmt})"
    assert got["written"] == want["written"], (what, got, want)
    if want["written"]:
        assert got == want, (what, got, want)
    else:
        assert all(l > h for l, h in zip(got["lo"], got["hi"])), (what, got)
    assert same_bits(got_d, want_d), what
    assert np.array_equal(got_m, want_m), what
    return want


@pytest.mark.parametrize("sfmt", K.FORMATS)
@pytest.mark.parametrize("dfmt", K.FORMATS)
@pytest.mark.parametrize("Ns", [9, 17])
@pytest.mark.parametrize("Nd", [17, 33])
def test_host_stamp_equals_the_reference_over_placements_and_ops(Nd, Ns, dfmt, sfmt):
    written = {}
    for case in K.sweep(Nd, Ns):
        written[case[0]] = check(case, Nd, Ns, dfmt, sfmt)["written"]
    assert all(n == 0 for what, n in written.items() if what.startswith("wholly outside"))
    for name in ("identity", "shift", "axis turn 0", "axis turn 5", "oblique 0", "oblique 1", "a source larger", "u lands on"):
        assert any(n > 0 for what, n in written.items() if what.startswith(name)), name  # the sweep is not vacuous there


@pytest.mark.parametrize("sfmt", K.FORMATS)
@pytest.mark.parametrize("dfmt", K.FORMATS)
def test_host_stamp_equals_the_reference_over_the_parameters(dfmt, sfmt):
    total = 0
    for case in K.parameter_cross(33, 17):
        total += check(case, 33, 17, dfmt, sfmt)["written"]
    assert total > 5000


def test_the_last_source_sample_is_reached_with_fraction_one():
    """Identity and the 0.5 scaling put destination samples on u = Ns - 1 exactly: cell Ns - 2, fraction 1, and the lerp returns the
    last sample's own value."""
    Nd, Ns = 17, 9
    src = K.volume("sphere", Ns, "src")
    for name, matrix, scale in K.placements(Nd, Ns):
        if name not in ("identity", "u lands on Ns - 1"):
            continue
        inside, t, ids = S.sample_source(src.density, src.material_id, R.F32, matrix, Nd)
        p = Ns - 1 if name == "identity" else 2 * (Ns - 1)
        assert inside[p, p, p] and (p + 1 >= Nd or not inside[p + 1, p, p])
        assert t[p, p, p].view(np.uint32) == src.density[Ns - 1, Ns - 1, Ns - 1].view(np.uint32)
        assert ids[p, p, p] == src.material_id[Ns - 1, Ns - 1, Ns - 1]


def test_replace_with_the_identity_copies_the_source():
    """Equal N, F32 into F32, equal metric, a finite field without +-0: the dense bits and, with MATERIAL_SOURCE, the ids."""
    N = 17
    src = K.volume("torus", N, "dst")
    assert np.isfinite(src.density).all() and (src.density != 0).all()
    dst = v.VVoxelVolume(K.RES[N], src.VolumeExtends)
    dst.density = K.hand_made(N, 5)
    rec = v.stamp_from_placement(N, ((N - 1) / 2.0,) * 3, op=_abi.STAMP_REPLACE, material=_abi.STAMP_MATERIAL_SOURCE)
    got = vx.stamp_host(dst, src, rec)
    assert got == {"written": N ** 3, "lo": (0, 0, 0), "hi": (N - 1,) * 3}
    assert same_bits(dst.density, src.density) and np.array_equal(dst.material_id, src.material_id)
    want_d, want_m = K.hand_made(N, 5), np.zeros((N,) * 3, np.uint8)
    S.apply(want_d, want_m, R.F32, src.VolumeExtends, 1.0, src.density, src.material_id, R.F32, src.VolumeExtends, 1.0, rec)
    assert same_bits(want_d, src.density) and np.array_equal(want_m, src.material_id)


def test_a_second_identical_hard_subtract_writes_nothing():
    Nd, Ns = 33, 17
    dst, src = K.volume("torus", Nd, "dst"), K.volume("sphere", Ns, "src")
    name, matrix, scale = K.placements(Nd, Ns)[9]
    rec = K.record(S.SUBTRACT, matrix, scale, 0.0, 0, 0.0)
    work = v.VVoxelVolume(K.RES[Nd], dst.VolumeExtends)
    work.density, work.material_id = np.array(dst.density), np.array(dst.material_id)
    want_d, want_m = np.array(dst.density), np.array(dst.material_id)
    want = S.apply(want_d, want_m, R.F32, dst.VolumeExtends, 1.0, src.density, src.material_id, R.F32, src.VolumeExtends, src.density_scale, rec)
    first = vx.stamp_host(work, src, rec)
    assert first == want and first["written"] > 100
    assert same_bits(work.density, want_d) and np.array_equal(work.material_id, want_m)
    second = vx.stamp_host(work, src, rec)
    assert second["written"] == 0 and all(l > h for l, h in zip(second["lo"], second["hi"]))
    assert same_bits(work.density, want_d) and np.array_equal(work.material_id, want_m)


def good_record():
    return v.stamp_record(_abi.STAMP_ADD, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], 1.0, 0.0, 0.0, 2.0, 3)


def refused_records():
    """[(what, record)]: one per VRT_ERR_INVALID rule of vrt.h that the record itself can break."""
    out = []

    def bad(what, **fields):
        r = good_record()
        for k, val in fields.items():
            if k[0] == "m" and k[1:].isdigit():
                r.dst_to_src[int(k[1:])] = val
            elif k == "reserved":
                r.reserved_[val] = 1
            else:
                setattr(r, k, val)
        out.append((what, r))

    bad("unknown op", op=3)
    bad("negative op", op=-1)
    bad("material 256", material=256)
    bad("material -3", material=-3)
    for name in ("length_scale", "offset", "blend", "reach"):
        for val in (math.nan, math.inf, -math.inf):
            bad(f"{name} {val}", **{name: val})
    for j in (0, 3, 7, 11):
        for val in (math.nan, math.inf):
            bad(f"matrix[{j}] {val}", **{f"m{j}": val})
    bad("length_scale 0", length_scale=0.0)
    bad("length_scale < 0", length_scale=-1.0)
    bad("blend < 0", blend=-0.5)
    bad("reach 0", reach=0.0)
    bad("reach < 0", reach=-1.0)
    bad("reach 0, SUBTRACT", reach=0.0, op=_abi.STAMP_SUBTRACT)
    for w in range(6):
        bad(f"reserved word {w}", reserved=w)
    bad("a zero row", m4=0.0, m5=0.0, m6=0.0)
    bad("two equal rows", m4=1.0, m5=0.0)
    bad("a zero matrix", m0=0.0, m5=0.0, m10=0.0)
    bad("a rank-2 oblique matrix", m0=1.0, m1=2.0, m2=3.0, m4=2.0, m5=4.0, m6=6.0, m8=0.5, m9=0.25, m10=1.0)
    return out


def accepted_records():
    out = []
    for name, fields in (("REPLACE ignores reach and blend beyond finiteness", dict(op=_abi.STAMP_REPLACE, reach=-1.0, blend=0.0)),
                         ("material 0", dict(material=0)), ("material 255", dict(material=255)),
                         ("KEEP", dict(material=_abi.STAMP_MATERIAL_KEEP)), ("SOURCE", dict(material=_abi.STAMP_MATERIAL_SOURCE)),
                         ("a negative offset", dict(offset=-3.0)), ("a mirror", dict()), ("a tiny regular matrix", dict())):
        r = good_record()
        for k, val in fields.items():
            setattr(r, k, val)
        if name == "a mirror":
            r.dst_to_src[0] = -1.0
        if name == "a tiny regular matrix":  # determinant 1e-90 in double: not 0, and its inverse is finite
            r.dst_to_src[0] = r.dst_to_src[5] = r.dst_to_src[10] = 1e-30
        out.append((name, r))
    return out


def test_argument_rules_without_a_gpu():
    """Through the C-ABI a NULL context or record is refused before anything else; every rule a record can break is checked by
    vrt_stamp_core::valid, which vrt_volume_stamp calls before it looks at a slot and which vrh_stamp reaches without a context (the
    same rules on a live context, and VRT_ERR_SLOT: tests/test_volume_stamp_gpu.py)."""
    lib = _abi.load()
    res = _abi.vrt_brush_result()
    good = good_record()
    assert lib.vrt_volume_stamp(None, 0, 1, C.byref(good), C.byref(res)) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_stamp(None, 0, 1, None, None) == _abi.VRT_ERR_INVALID
    host = vx.load_host()
    d, s = np.zeros(27, VOXEL), np.zeros(27, VOXEL)
    call = lambda rec, dst=d, src=s: host.vrh_stamp(dst.ctypes.data if dst is not None else None, 3, 1.0, 1.0, 0,
                                                    src.ctypes.data if src is not None else None, 3, 1.0, 1.0, 0, rec, C.byref(res))
    assert call(C.byref(good)) == _abi.VRT_OK
    assert call(None) == _abi.VRT_ERR_INVALID
    assert call(C.byref(good), dst=None) == _abi.VRT_ERR_INVALID and call(C.byref(good), src=None) == _abi.VRT_ERR_INVALID
    assert call(C.byref(good), src=d) == _abi.VRT_ERR_INVALID  # a volume into itself: dst_slot == src_slot
    for what, rec in refused_records():
        assert call(C.byref(rec)) == _abi.VRT_ERR_INVALID, what
    for what, rec in accepted_records():
        assert call(C.byref(rec)) == _abi.VRT_OK, what


def test_stamp_record_has_the_c_layout(tmp_path):
    fields = ("op", "material", "dst_to_src", "length_scale", "offset", "blend", "reach", "reserved_")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\nint main(void){\nprintf("%zu", sizeof(vrt_stamp));\n'
                    + "".join(f'printf(" %zu", offsetof(vrt_stamp, {f}));\n' for f in fields)
                    + 'printf(" %d %d %d %d %d\\n", VRT_STAMP_ADD, VRT_STAMP_SUBTRACT, VRT_STAMP_REPLACE, VRT_STAMP_MATERIAL_KEEP,'
                    " VRT_STAMP_MATERIAL_SOURCE);\nreturn 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_abi.vrt_stamp)] + [getattr(_abi.vrt_stamp, f).offset for f in fields]
    want += [_abi.STAMP_ADD, _abi.STAMP_SUBTRACT, _abi.STAMP_REPLACE, _abi.STAMP_MATERIAL_KEEP, _abi.STAMP_MATERIAL_SOURCE]
    assert got == want and got[0] == 96
    assert (S.ADD, S.SUBTRACT, S.REPLACE, S.KEEP, S.SOURCE) == tuple(want[-5:])
    assert "vrt_volume_stamp" in _abi.SYMBOLS


def test_stamp_from_placement():
    for N in (9, 33):
        rec = v.stamp_from_placement(N, (0.0, 0.0, 0.0))
        c = (N - 1) / 2.0
        assert list(rec.dst_to_src) == [1, 0, 0, c, 0, 1, 0, c, 0, 0, 1, c]  # the centring matrix
        assert (rec.op, rec.material, rec.length_scale, rec.offset, rec.blend) == (_abi.STAMP_ADD, _abi.STAMP_MATERIAL_KEEP, 1.0, 0.0, 0.0)
    # a quarter turn about z at scale 2, centre on (10, 20, 30): destination +x is source +y... the source's axes turn with R
    rec = v.stamp_from_placement(17, (10.0, 20.0, 30.0), K.quat((0, 0, 1), 90.0), 2.0, op=_abi.STAMP_SUBTRACT, material=4)
    m = np.array(list(rec.dst_to_src), np.float64).reshape(3, 4)
    assert np.allclose(m[:, :3], np.array([[0, 0.5, 0], [-0.5, 0, 0], [0, 0, 0.5]]), atol=1e-7)
    assert np.allclose(m @ np.array([10.0, 20.0, 30.0, 1.0]), 8.0, atol=1e-5)  # the placement's position is the source's centre sample
    assert rec.length_scale == 2.0 and rec.op == _abi.STAMP_SUBTRACT and rec.material == 4
    assert np.allclose(1.0 / np.linalg.norm(m[:, :3], axis=1), rec.length_scale)  # 1 / |row| for a similarity
    with pytest.raises(ValueError):
        v.stamp_from_placement(17, (0, 0, 0), scale=0.0)
