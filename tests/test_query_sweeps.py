"""Sweep queries (vrt_query_sweeps / _host) without a GPU: argument errors come back before any device work, the record layouts of C,
ctypes and numpy agree, and the numpy restatement of the rule (sweep_ref.py), which the GPU tests compare the kernel with, is itself
worth something — on an analytic sphere it hits what the sphere grown by the radius says it should, a little late, by the trilinear
sag; a sweep is its evaluations chained through the point query; and on the inputs of the GPU test the float64 reference leaves few
enough records undecided."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import capacity_scenes as cs
import points_ref as P
import sweep_cases as K
import sweep_ref as S
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_argument_errors_without_touching_the_gpu():
    lib = _abi.load()
    rec = np.zeros(4, v.SWEEP_DTYPE)
    res = np.zeros(4, v.SWEEP_HIT_DTYPE)
    sp, rp = rec.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)
    INVALID = _abi.VRT_ERR_INVALID
    assert lib.vrt_query_sweeps(None, 8, 0.0, 1e-3, 4, sp, rp, None) == INVALID
    assert lib.vrt_query_sweeps_host(None, 8, 0.0, 1e-3, 4, sp, rp) == INVALID
    assert lib.vrt_query_sweeps(None, 8, 0.0, 1e-3, 0, None, None, None) == INVALID
    # The remaining rules are checked before the context is looked at, and without a scene that look reads one flag: a block of zero
    # bytes can stand in for a context that has no device and no scene.
    blank = (C.c_uint8 * (8 << 20))()
    ctx = C.cast(blank, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    for device_form in (True, False):
        def call(max_steps, tolerance, step_min, n, s, r):
            if device_form:
                return lib.vrt_query_sweeps(ctx, max_steps, tolerance, step_min, n, s, r, None)
            return lib.vrt_query_sweeps_host(ctx, max_steps, tolerance, step_min, n, s, r)
        assert call(8, 0.0, 1e-3, -1, sp, rp) == INVALID
        assert call(8, 0.0, 1e-3, 4, None, rp) == INVALID
        assert call(8, 0.0, 1e-3, 4, sp, None) == INVALID
        for steps in (0, -1, _abi.MAX_SWEEP_STEPS + 1):
            assert call(steps, 0.0, 1e-3, 4, sp, rp) == INVALID
        for tol in (-1e-6, nan, inf, -inf):
            assert call(8, tol, 1e-3, 4, sp, rp) == INVALID
            assert call(8, tol, 1e-3, 0, None, None) == INVALID
        for step_min in (0.0, -0.0, -1e-3, nan, inf, -inf):
            assert call(8, 0.0, step_min, 4, sp, rp) == INVALID
            assert call(8, 0.0, step_min, 0, None, None) == INVALID
        # nothing wrong with the arguments: no scene
        assert call(1, 0.0, 1e-3, 4, sp, rp) == _abi.VRT_ERR_NOT_READY
        assert call(_abi.MAX_SWEEP_STEPS, 0.5, 1e-30, 0, None, None) == _abi.VRT_ERR_NOT_READY
    assert not res.view(np.uint8).any()  # nothing written


def test_sweep_records_have_the_c_layout(tmp_path):
    fields = ["sizeof(vrt_sweep)", "offsetof(vrt_sweep, origin)", "offsetof(vrt_sweep, t_max)", "offsetof(vrt_sweep, direction)",
              "offsetof(vrt_sweep, radius)", "sizeof(vrt_sweep_hit)", "offsetof(vrt_sweep_hit, t)", "offsetof(vrt_sweep_hit, normal)",
              "offsetof(vrt_sweep_hit, instance)", "offsetof(vrt_sweep_hit, voxel)", "offsetof(vrt_sweep_hit, material)",
              "offsetof(vrt_sweep_hit, flags)", "offsetof(vrt_sweep_hit, steps)", "offsetof(vrt_sweep_hit, distance)",
              "offsetof(vrt_sweep_hit, position)", "offsetof(vrt_sweep_hit, reserved_)", "VRT_MAX_SWEEP_STEPS", "VRT_SWEEP_HIT",
              "VRT_SWEEP_EXHAUSTED", "VRT_SWEEP_INITIAL"]
    prog = tmp_path / "p.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\nint main(void){\n' +
                    "".join(f'printf("%ld\\n", (long)({f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    Q, R = _abi.vrt_sweep, _abi.vrt_sweep_hit
    want = [C.sizeof(Q), Q.origin.offset, Q.t_max.offset, Q.direction.offset, Q.radius.offset, C.sizeof(R), R.t.offset, R.normal.offset,
            R.instance.offset, R.voxel.offset, R.material.offset, R.flags.offset, R.steps.offset, R.distance.offset, R.position.offset,
            R.reserved_.offset, _abi.MAX_SWEEP_STEPS, _abi.SWEEP_HIT, _abi.SWEEP_EXHAUSTED, _abi.SWEEP_INITIAL]
    assert got == want
    assert got[0] == 32 and got[5] == 64 and got[14] == 48 and got[16:] == [4096, 1, 2, 4]
    assert v.SWEEP_DTYPE.itemsize == 32 and v.SWEEP_HIT_DTYPE.itemsize == 64
    assert [v.SWEEP_DTYPE.fields[n][1] for n in ("origin", "t_max", "direction", "radius")] == got[1:5]
    names = ("t", "normal", "instance", "voxel", "material", "flags", "steps", "distance", "position", "reserved_")
    assert [v.SWEEP_HIT_DTYPE.fields[n][1] for n in names] == got[6:16]
    assert (S.HIT, S.EXHAUSTED, S.INITIAL) == (_abi.SWEEP_HIT, _abi.SWEEP_EXHAUSTED, _abi.SWEEP_INITIAL)


# ---- the reference's own worth: the analytic spheres of test_query_points.py, cells of 1 ---------------------------------------------
GRAZING_BAND = 0.1                 # cells: nearer than this to grazing the grown sphere, the reference and the sphere may disagree on a hit
STATED_LATE = {9: 0.45, 17: 0.28}  # cells, measured here (0.425 and 0.263) and stated in DESIGN.md: how late a hit outside the band is


@pytest.fixture(scope="module")
def sphere_sweeps():
    """(N, radius) -> (records, sweep_ref's records, b, R, t*): the impact parameter, the grown sphere's radius, the analytic t."""
    out = {}
    for N in sorted(K.SPHERES):
        for radius in (0.0, 0.5, 1.0):
            rec = K.sphere_records(N, radius)
            got = S.sweep([K.sphere_slot(N)], [P.Instance(0)], rec, K.SPHERE_STEPS, K.SPHERE_TOLERANCE, K.SPHERE_STEP_MIN)
            o, d = rec["origin"].astype(np.float64), rec["direction"].astype(np.float64)
            u = d / np.linalg.norm(d, axis=1, keepdims=True)
            tc = -(o * u).sum(axis=1)
            b = np.linalg.norm(o + u * tc[:, None], axis=1)
            R = K.SPHERES[N] + radius
            out[N, radius] = (rec, got, b, R, tc - np.sqrt(np.maximum(R * R - b * b, 0.0)))
    return out


@pytest.mark.parametrize("radius", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N", sorted(K.SPHERES))
def test_reference_hits_the_grown_sphere_a_little_late(sphere_sweeps, N, radius):
    rec, got, b, R, t_star = sphere_sweeps[N, radius]
    hit = (got["flags"] & S.HIT) != 0
    exhausted = (got["flags"] & S.EXHAUSTED) != 0
    assert hit.sum() > 2000 and (~hit & ~exhausted).sum() > 50 and not (got["flags"] & S.INITIAL).any()
    steps = got["steps"][hit]
    print(f"N {N} radius {radius}: {int(hit.sum())} hits, {int(exhausted.sum())} exhausted, median {np.median(steps):.0f} evaluations per hit, "
          f"largest {int(got['steps'].max())}")
    assert 8 <= np.median(steps) <= 20
    clear = np.abs(b - R) > GRAZING_BAND
    decided = clear & ~exhausted
    assert np.array_equal(hit[decided], (b < R)[decided])
    assert (b[exhausted] > R - GRAZING_BAND).all() if exhausted.any() else True  # only a grazing record runs out of steps
    # a hit is never early by more than the tolerance allows: the interpolant of a convex field never undershoots it, so c <= tolerance
    # says that the true clearance is <= tolerance too, and the centre is at most that far outside the grown sphere
    sure = hit & clear
    early = np.sqrt((R + K.SPHERE_TOLERANCE) ** 2 - b[sure] ** 2) - np.sqrt(R * R - b[sure] ** 2)
    late = got["t"][sure].astype(np.float64) - t_star[sure]
    print(f"   outside the grazing band: late by {late.min():.4f} .. {late.max():.3f} cells")
    assert np.all(late >= -early - 1e-5)
    # late, by what the interpolant overshoots (the steps are as long as it says), over the cosine at impact: measured, see DESIGN.md
    assert late.max() <= STATED_LATE[N]
    # at every HIT the point query's rule at `position` says so
    at = P.evaluate([K.sphere_slot(N)], [P.Instance(0)], got["position"][hit])
    assert at["sampled"].all() and np.all(at["distance"] - f32(radius) <= f32(K.SPHERE_TOLERANCE))
    assert np.array_equal(at["distance"].view(np.uint32), got["distance"][hit].view(np.uint32))
    assert np.array_equal(at["normal"].view(np.uint32), got["normal"][hit].view(np.uint32)) and np.array_equal(at["voxel"], got["voxel"][hit])


def test_all_three_outcomes_occur_on_the_spheres(sphere_sweeps):
    flags = np.concatenate([got["flags"] for _, got, _, _, _ in sphere_sweeps.values()])
    assert ((flags & S.HIT) != 0).any() and ((flags & S.EXHAUSTED) != 0).any() and (flags == 0).any()


@pytest.mark.parametrize("max_steps", [1, 3, 64])
def test_a_sweep_is_its_evaluations_chained_through_the_point_query(max_steps):
    slots, inst = K.ref_scene(K.placed_one_scene())
    rec = K.placed_one_records()
    got = S.sweep(slots, inst, rec, max_steps, 1e-3, 1e-2)
    assert (~got["cand"][:, 0]).sum() > 20
    want = S.chain(lambda p: P.query(slots, inst, p), got["cand"][:, 0], rec, max_steps, 1e-3, 1e-2)
    assert S.same_bits(got, want) == []
    hit = (got["flags"] & S.HIT) != 0
    assert hit.any() and ((got["flags"] & S.EXHAUSTED) != 0).any() and (got["flags"] == 0).any()
    assert (got["steps"] <= max_steps).all()


def test_reference_records_off_the_hit_path():
    sc, vol = K.pinned_scene(3, _abi.FORMAT_F32, "sphere")
    slots, inst = K.ref_scene(sc)
    rec = K.pinned_records(vol, 3)
    got = S.sweep(slots, inst, rec, 256, 1e-3, 0.01 * vol.GetCellSize())
    bad = slice(len(rec) - K.BAD, None)
    assert (got["steps"][bad] == 0).all() and (got["flags"][bad] == 0).all() and (got["t"][bad] == -1).all()
    assert np.array_equal(got["position"][bad].view(np.uint32), rec["origin"][bad].view(np.uint32))
    assert (got["steps"][:-K.BAD] >= 1).all()
    miss = got["flags"] == 0
    assert (got["t"][miss] == -1).all() and np.isposinf(got["distance"][miss]).all() and (got["instance"][miss] == -1).all()
    assert (got["voxel"][miss] == -1).all() and (got["normal"][miss] == 0).all() and (got["material"][miss] == 0).all()
    initial = (got["flags"] & S.INITIAL) != 0
    assert initial.any() and (got["steps"][initial] == 1).all() and (got["t"][initial] == 0).all()
    zero = rec["t_max"] == 0
    assert zero.sum() > 10 and (got["steps"][zero] == 1).all()  # t_max 0: one evaluation, at the origin


# ---- the inputs of the GPU test: the float64 reference decides all but a few records ---------------------------------------------------
def relative(a, b):
    """|a - b| over max(1, |b|), where both are finite."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    return np.where(ok, np.abs(a - np.where(ok, b, 0.0)) / np.maximum(1.0, np.abs(np.where(ok, b, 0.0))), 0.0)


def test_the_placed_inputs_leave_few_records_ambiguous_and_the_references_agree_within_the_stated_figure():
    slots, inst = K.ref_scene(K.placed_scene())
    rec = K.placed_records()
    args = (K.PLACED_STEPS, K.PLACED_TOLERANCE, K.PLACED_STEP_MIN)
    want = S.sweep(slots, inst, rec, *args, dtype=np.float64, margin=K.PLACED_MARGIN)
    share = want["ambiguous"].mean()
    print(f"{len(rec)} records: {share:.2%} ambiguous")
    assert share < K.AMBIGUOUS_CAP
    fp32 = S.sweep(slots, inst, rec, *args)
    ok = ~want["ambiguous"]
    for key in S.INTS:
        assert np.array_equal(np.asarray(fp32[key])[ok], np.asarray(want[key])[ok]), key
    hit = ok & ((want["flags"] & S.HIT) != 0)
    worst = max(relative(fp32["t"][hit], want["t"][hit]).max(), relative(fp32["distance"][hit], want["distance"][hit]).max(),
                np.abs(fp32["normal"][hit].astype(np.float64) - want["normal"][hit]).max())
    print(f"largest fp32 / fp64 difference of t, distance (relative to max(1, |x|)) and normal: {worst:.2e}")
    assert worst <= K.PLACED_REF_DIFFERENCE
    assert hit.sum() > 500 and set(want["instance"][hit].tolist()) == {0, 1, 2}
    assert (~want["cand"]).any(axis=1).mean() > 0.3  # many records leave an instance out


def test_the_lattice_inputs_leave_few_records_ambiguous():
    slots, inst = K.ref_scene(cs.lattice64("mixed"))
    rec = K.lattice_records()
    want = S.sweep(slots, inst, rec, K.LATTICE_STEPS, K.LATTICE_TOLERANCE, K.LATTICE_STEP_MIN, dtype=np.float64, margin=K.LATTICE_MARGIN)
    print(f"{len(rec)} records: {want['ambiguous'].mean():.2%} ambiguous")
    assert want["ambiguous"].mean() < K.AMBIGUOUS_CAP
    hit = ~want["ambiguous"] & ((want["flags"] & S.HIT) != 0)
    assert len(set(want["instance"][hit].tolist())) > 40
    assert ((~want["cand"]).sum(axis=1) > 32).any()
