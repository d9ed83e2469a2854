"""Contact queries (vrt_query_contacts) without a GPU: argument errors come back before any device work, the record layouts of C, ctypes
and numpy agree, the host pass (VVolumeConverter::Contacts through libvrt_host.so's vrh_contacts, built from the same contacts_core.h as
the kernels) equals the numpy restatement of the rule (contacts_ref.py) bit for bit on every case of contacts_cases.py, with and without
the conservative cell box, and that restatement is itself worth something: on two overlapping spheres the deepest distance is the
analytic overlap up to the two surfaces' sag and the deepest contact's normal follows the line of centres."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contacts_cases as CC
import contacts_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi, voxelizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def host(a, b, margin, clip=True):
    return voxelizer.contacts_host(a.stored, a.material, a.placed(), b.stored, b.material, b.placed(), margin, clip=clip)


def test_argument_errors_without_touching_the_gpu():
    lib = _abi.load()
    rec = np.zeros(4, v.CONTACT_DTYPE)
    res = _abi.vrt_contacts_result()
    rp, out = rec.ctypes.data_as(C.c_void_p), C.byref(res)
    INVALID = _abi.VRT_ERR_INVALID
    assert lib.vrt_query_contacts(None, 0, 1, 0.0, rp, 4, out) == INVALID
    assert lib.vrt_query_contacts(None, 0, 1, 0.0, None, 0, out) == INVALID
    # The remaining rules are checked before the context is looked at, and without a scene that look reads one flag: a block of zero
    # bytes can stand in for a context that has no device and no scene (test_query_points.py does the same).
    blank = (C.c_uint8 * (8 << 20))()
    ctx = C.cast(blank, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    assert lib.vrt_query_contacts(ctx, 0, 1, 0.0, rp, 4, None) == INVALID
    for margin in (-1e-6, nan, inf, -inf):
        assert lib.vrt_query_contacts(ctx, 0, 1, margin, rp, 4, out) == INVALID
        assert lib.vrt_query_contacts(ctx, 0, 1, margin, None, 0, out) == INVALID
    assert lib.vrt_query_contacts(ctx, 1, 1, 0.0, rp, 4, out) == INVALID
    assert lib.vrt_query_contacts(ctx, 0, 0, 0.5, None, 0, out) == INVALID
    assert lib.vrt_query_contacts(ctx, 0, 1, 0.0, None, 1, out) == INVALID
    # nothing wrong with the arguments: no scene
    assert lib.vrt_query_contacts(ctx, 0, 1, 0.0, rp, 4, out) == _abi.VRT_ERR_NOT_READY
    assert lib.vrt_query_contacts(ctx, 5, 2, 0.25, None, 0, out) == _abi.VRT_ERR_NOT_READY
    assert not rec.view(np.uint8).any() and bytes(res) == bytes(C.sizeof(res))  # nothing written


def test_contact_records_have_the_c_layout(tmp_path):
    fields = ["sizeof(vrt_contact)", "offsetof(vrt_contact, position)", "offsetof(vrt_contact, distance)", "offsetof(vrt_contact, normal)",
              "offsetof(vrt_contact, material_a)", "offsetof(vrt_contact, normal_a)", "offsetof(vrt_contact, material_b)",
              "offsetof(vrt_contact, cell_a)", "offsetof(vrt_contact, reserved_)", "sizeof(vrt_contacts_result)",
              "offsetof(vrt_contacts_result, lo)", "offsetof(vrt_contacts_result, hi)", "offsetof(vrt_contacts_result, contacts)",
              "offsetof(vrt_contacts_result, candidates)", "offsetof(vrt_contacts_result, min_distance)",
              "offsetof(vrt_contacts_result, reserved_)"]
    prog = tmp_path / "c.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\nint main(void){\n' +
                    "".join(f'printf("%ld\\n", (long)({f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "c"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    K, S = _abi.vrt_contact, _abi.vrt_contacts_result
    want = [C.sizeof(K), K.position.offset, K.distance.offset, K.normal.offset, K.material_a.offset, K.normal_a.offset, K.material_b.offset,
            K.cell_a.offset, K.reserved_.offset, C.sizeof(S), S.lo.offset, S.hi.offset, S.contacts.offset, S.candidates.offset,
            S.min_distance.offset, S.reserved_.offset]
    assert got == want
    assert got[0] == 64 and got[9] == 48
    assert got[1:9] == [0, 12, 16, 28, 32, 44, 48, 60]  # four 16-byte words
    names = ("position", "distance", "normal", "material_a", "normal_a", "material_b", "cell_a", "reserved_")
    assert v.CONTACT_DTYPE.itemsize == 64 and [v.CONTACT_DTYPE.fields[n][1] for n in names] == got[1:9]


@pytest.mark.parametrize("case", sorted(CC.CASES))
def test_the_host_pass_equals_the_restatement_bit_for_bit(case):
    a, b = CC.CASES[case]()
    for margin in CC.margins(a):
        want = R.contacts(a.slot(), a.inst(), b.slot(), b.inst(), margin)
        got = host(a, b, margin)
        print(f"{case} margin {margin:.4f}: {want['candidates']} candidates, {want['contacts']} contacts, deepest {want['min_distance']:.4f}")
        assert R.same_bits(got, want) == []
        assert (got["contacts"] == 0) == (case in CC.EMPTY) and (got["candidates"] == 0) == (case in CC.EMPTY)  # no case is vacuous
        assert got["contacts"] == len(got["distance"]) <= got["candidates"]
        if got["contacts"]:
            assert np.all(got["distance"] <= f32(margin)) and got["min_distance"] == got["distance"].min()
            key = (got["cell_a"][:, 0].astype(np.int64) * a.N + got["cell_a"][:, 2]) * a.N + got["cell_a"][:, 1]
            assert np.all(np.diff(key) > 0)  # the order of the cells' keys
        # the conservative cell box changes nothing: the same bytes from all of A's cells
        assert R.same_bits(host(a, b, margin, clip=False), got) == []


def test_what_the_cases_hold():
    # margin only adds contacts; candidates do not depend on it
    a, b = CC.CASES["spheres17_overlap1"]()
    tight, wide = (host(a, b, m) for m in CC.margins(a))
    assert tight["candidates"] == wide["candidates"] and tight["contacts"] < wide["contacts"]
    assert set(map(tuple, tight["cell_a"])) < set(map(tuple, wide["cell_a"]))
    # a NaN sample of B: the cells around it give no candidate
    clean, holed = host(a, b, 0.0), host(*CC.CASES["nan_in_b"](), 0.0)
    assert 0 < holed["candidates"] < clean["candidates"] and 0 < holed["contacts"] < clean["contacts"]
    # B wholly containing A: every vertex of A is a candidate and a contact, all inside
    a, b = CC.CASES["b_contains_a"]()
    got = host(a, b, 0.0)
    assert got["contacts"] == got["candidates"] == len(R.active_cells(a.stored, a.fmt)) and np.all(got["distance"] < 0)
    # B's box over one corner of A only
    a, b = CC.CASES["corner_only"]()
    got = host(a, b, 0.0)
    assert got["contacts"] > 0 and min(got["lo"]) >= a.N // 2 and got["candidates"] < len(R.active_cells(a.stored, a.fmt)) // 4
    # the two instances may share a volume; the call is one-sided: swapping the sides gives B's surface points
    a, b = CC.CASES["spheres9_overlap1"]()
    b.density, b.material = a.density, a.material
    one, other = host(a, b, 0.0), host(b, a, 0.0)
    assert one["contacts"] > 0 and other["contacts"] > 0 and R.same_bits(other, R.contacts(b.slot(), b.inst(), a.slot(), a.inst(), 0.0)) == []
    assert not np.array_equal(one["position"][:1], other["position"][:1])


def test_count_then_fetch_and_a_capacity_too_small():
    lib = voxelizer.load_host()
    a, b = CC.CASES["spheres17_overlap1"]()
    keep = []

    def side(s):
        rec = np.zeros(s.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        rec["density"], rec["material"] = s.stored.reshape(-1), s.material.reshape(-1)
        keep.append(rec)
        p = s.placed()
        return voxelizer.vrh_placed_volume(rec.ctypes.data, s.N, int(p["texel16"]), p["extent"], p["density_scale"], p["step_max"],
                                           (C.c_float * 3)(*p["position"]), (C.c_float * 4)(*p["rotation"]), (C.c_float * 3)(*p["scale"]))

    A, B = side(a), side(b)
    res = _abi.vrt_contacts_result()
    assert lib.vrh_contacts(C.byref(A), C.byref(B), 0.0, 1, None, 0, C.byref(res)) == 0  # count only
    n = int(res.contacts)
    assert n == 21 and res.candidates == 194
    rec = np.frombuffer(bytearray(b"\xab" * (64 * n)), v.CONTACT_DTYPE)
    before = rec.tobytes()
    res2 = _abi.vrt_contacts_result()
    assert lib.vrh_contacts(C.byref(A), C.byref(B), 0.0, 1, rec.ctypes.data, n - 1, C.byref(res2)) == -2
    assert rec.tobytes() == before and bytes(res2) == bytes(res)  # the result is filled, no byte of the records touched
    assert lib.vrh_contacts(C.byref(A), C.byref(B), 0.0, 1, rec.ctypes.data, n, C.byref(res2)) == 0
    assert rec.tobytes() != before and (rec["reserved_"] == 0).all()
    assert lib.vrh_contacts(C.byref(A), C.byref(B), 0.0, 1, None, 3, C.byref(res2)) == -1  # NULL records with a capacity
    assert lib.vrh_contacts(C.byref(A), C.byref(B), -1.0, 1, None, 0, C.byref(res2)) == -1
    assert lib.vrh_contacts(C.byref(A), None, 0.0, 1, None, 0, C.byref(res2)) == -1


# ---- the reference's own worth: two analytic spheres --------------------------------------------------------------------------------
# What DESIGN.md states ("what the rule is worth"), measured here: the deepest distance against the analytic overlap, in cells of A,
# and the angle between the deepest contact's normal (B's, inside -> outside) and the line from B's centre to A's.
WORTH = {  # N: (overlap in cells, |deepest + overlap| in cells, angle in degrees) as stated; measured: 0.257 / 14.28, 0.121 / 6.98, 0.053 / 0.71
    9: (1.0, 0.30, 15.0),
    17: (1.0, 0.15, 7.5),
    33: (1.0, 0.08, 3.0),
}


@pytest.mark.parametrize("N", sorted(WORTH))
def test_the_deepest_contact_is_the_analytic_overlap_up_to_the_sag(N):
    overlap, tol_cells, tol_angle = WORTH[N]
    a, b = CC.pair(N, N, overlap)
    got = R.contacts(a.slot(), a.inst(), b.slot(), b.inst(), 0.0)
    cell = 2.0 / (N - 1)
    deepest = int(np.argmin(got["distance"]))
    line = a.world_centre() - b.world_centre()
    line /= np.linalg.norm(line)
    cos = float(np.dot(got["normal"][deepest].astype(np.float64), line))
    angle = np.degrees(np.arccos(min(1.0, cos)))
    print(f"N {N}: {got['contacts']} contacts of {got['candidates']} candidates, deepest {got['min_distance'] / cell:.3f} cells "
          f"(analytic {-overlap:.2f}), normal {angle:.2f} degrees off the line of centres")
    # a vertex of A lies up to its sag inside A's sphere and B's interpolant reads up to its sag high (both < cell^2 / (8 r) * 3), and the
    # deepest VERTEX lies up to half a cell diagonal off the line of centres, where B's surface has curved away by about d^2 / (2 r)
    assert abs(got["min_distance"] / cell + overlap) <= tol_cells
    assert got["min_distance"] > -overlap * cell  # never deeper than the analytic overlap: both errors read shallow
    assert angle <= tol_angle
