"""GPU contact queries (vrt_query_contacts, VHipRenderer.query_contacts) against the numpy restatement of the rule (contacts_ref.py) and
against the host pass (vrh_contacts), bit for bit, on the cases of contacts_cases.py and at the grid sizes where the kernels take
another path; the composition the header states (a contact's distance, normal and material_b are vrt_query_points of its position in a
scene that holds B alone; its position is the fp32 transform of vrt_volume_extract_mesh's vertex); and as plumbing: nothing of either
slot or of the render's bookkeeping moves, a deferred scene set is honoured, bad indices and a short capacity are refused."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import contacts_cases as CC
import contacts_ref as R
import points_ref as P
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi, voxelizer

pytestmark = pytest.mark.gpu
f32 = np.float32
WHICH = {"dense": _abi.VOLUME_BYTES_DENSE, "material": _abi.VOLUME_BYTES_MATERIAL, "bricks": _abi.VOLUME_BYTES_BRICKS,
         "cells": _abi.VOLUME_BYTES_CELLS, "skip": _abi.VOLUME_BYTES_SKIP, "nib": _abi.VOLUME_BYTES_NIB,
         "cube_skip": _abi.VOLUME_BYTES_CUBE_SKIP, "active_box": _abi.VOLUME_BYTES_ACTIVE_BOX}


@pytest.fixture(scope="module")
def cq():
    """A context of this module's own (the session renderer's scene and output size stay as other modules left them)."""
    with v.VHipRenderer() as r:
        yield r


def volume_of(side: CC.Side) -> v.VVoxelVolume:
    vol = v.VVoxelVolume(int(np.log2(side.N - 1)), side.extent)
    assert vol.N == side.N
    vol.density = np.ascontiguousarray(side.density, f32)
    vol.material_id = np.ascontiguousarray(side.material, np.uint8)
    vol.density_scale, vol.step_max = side.density_scale, side.step_max
    return vol.set_device_format(side.fmt)


def placed(side: CC.Side, vol) -> v.VVoxelObject:
    return v.VVoxelObject(Position=tuple(side.position), Rotation=tuple(side.rotation), Scale=tuple(side.scale), Volume=vol)


def use(r, a: CC.Side, b: CC.Side) -> v.VScene:
    sc = v.VScene(Objects=[placed(a, volume_of(a)), placed(b, volume_of(b))])
    r.SetSceneToRender(sc)
    r.SyncWithScene()
    return sc


def reference(a, b, margin):
    return R.contacts(a.slot(), a.inst(), b.slot(), b.inst(), margin)


def host(a, b, margin):
    return voxelizer.contacts_host(a.stored, a.material, a.placed(), b.stored, b.material, b.placed(), margin)


def buffers(r, slot, device=0):
    out = {}
    for name, which in WHICH.items():
        size = C.c_size_t(0)
        _abi.check(r._lib.vrt_debug_volume_bytes(r._ctx, slot, device, which, None, 0, C.byref(size)), "vrt_debug_volume_bytes")
        buf = np.zeros(size.value, np.uint8)
        _abi.check(r._lib.vrt_debug_volume_bytes(r._ctx, slot, device, which, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(size)),
                   "vrt_debug_volume_bytes")
        out[name] = buf
    return out


# -- 1. the cases, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CC.CASES))
def test_the_device_equals_the_restatement_and_the_host_pass(cq, case):
    a, b = CC.CASES[case]()
    use(cq, a, b)
    for margin in CC.margins(a):
        got = cq.query_contacts(0, 1, margin)
        want = reference(a, b, margin)
        print(f"{case} margin {margin:.4f}: {got['candidates']} candidates, {got['contacts']} contacts, deepest {got['min_distance']:.4f}")
        assert R.same_bits(got, want) == []
        assert R.same_bits(got, host(a, b, margin)) == []
        assert (got["contacts"] == 0) == (case in CC.EMPTY)


def test_one_sided_and_two_instances_of_one_slot(cq):
    a, b = CC.CASES["spheres17_overlap1"]()
    b.density, b.material = a.density, a.material
    vol = volume_of(a)
    sc = v.VScene(Objects=[placed(a, vol), placed(b, vol)])
    cq.SetSceneToRender(sc)
    cq.SyncWithScene()
    one, other = cq.query_contacts(0, 1), cq.query_contacts(1, 0)
    assert one["contacts"] > 0 and other["contacts"] > 0
    assert R.same_bits(one, reference(a, b, 0.0)) == [] and R.same_bits(other, reference(b, a, 0.0)) == []


# -- 2. the composition the header states ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["b_scaled_rotated", "a_scaled_rotated", "texel16_both", "step_max_and_scale"])
def test_a_contact_is_query_points_of_its_position_and_the_transform_of_the_mesh_vertex(cq, case):
    a, b = CC.CASES[case]()
    sc = use(cq, a, b)
    got = cq.query_contacts(0, 1, CC.margins(a)[1])
    assert got["contacts"] > 10
    # position: vrt_volume_extract_mesh's vertices of A's slot, through step 2 in fp32, at the contacts' cells
    positions, normals, materials, _, info = cq.extract_mesh(0)
    cells = R.active_cells(a.stored, a.fmt)  # the vertices' cells, in the vertices' order
    assert len(cells) == info["vertices"]
    key = lambda c: (c[:, 0].astype(np.int64) * a.N + c[:, 2]) * a.N + c[:, 1]
    at = np.searchsorted(key(cells), key(got["cell_a"]))
    assert np.array_equal(cells[at], got["cell_a"])
    O, pos = R.pack_o2w(a.rotation, a.scale), np.asarray(a.position, f32)
    o = positions[at].astype(f32)
    w = np.stack([(((O[i, 0] * o[:, 0] + O[i, 1] * o[:, 1]).astype(f32) + O[i, 2] * o[:, 2]).astype(f32) + pos[i]).astype(f32) for i in range(3)], axis=1)
    assert np.array_equal(w.view(np.uint32), got["position"].view(np.uint32))
    assert np.array_equal(materials[at].astype(np.uint32), got["material_a"])
    # distance, normal, material_b: vrt_query_points in a scene that holds B alone
    alone = v.VScene(Objects=[sc.Objects[1]])
    cq.SetSceneToRender(alone)
    rec = cq.query_points(got["position"])
    assert rec["sampled"].all() and (rec["instance"] == 0).all()
    for field, other in (("distance", "distance"), ("normal", "normal")):
        assert np.array_equal(rec[other].view(np.uint32), got[field].view(np.uint32)), field
    assert np.array_equal(rec["material"], got["material_b"])


# -- 3. the shapes where the kernels can go wrong ----------------------------------------------------------------------------------------
def test_n33_a_partial_run_of_32_cells(cq):
    a, b = CC.b_contains_a(33)  # the clipped box is all of A: rows of 32 cells, half a run
    use(cq, a, b)
    got = cq.query_contacts(0, 1)
    assert R.same_bits(got, reference(a, b, 0.0)) == []
    assert got["contacts"] == got["candidates"] == len(R.active_cells(a.stored, a.fmt)) > 1000


def test_n65_one_run_per_row_and_more_runs_than_a_scan_block(cq):
    a, b = CC.b_contains_a(65)  # 64 x 64 rows of exactly one run: 4096 runs, two scan blocks of 2048
    use(cq, a, b)
    got = cq.query_contacts(0, 1)
    want = reference(a, b, 0.0)
    assert R.same_bits(got, want) == []
    assert got["contacts"] == len(R.active_cells(a.stored, a.fmt)) > 5000
    run = got["cell_a"][:, 0] * 64 + got["cell_a"][:, 2]  # the clipped box is all of A: a row's run number
    assert (run < 2048).sum() > 1000 and (run >= 2048).sum() > 1000  # contacts on either side of the scan blocks' boundary
    assert R.same_bits(got, host(a, b, 0.0)) == []


def test_n129_a_patch_across_the_boundary_of_two_runs(cq):
    a = CC.sphere(129, radius_cells=40.3)
    b = CC.sphere(17, centre=(-0.011, 0.019, 0.023), seed=2, rotation=CC.QUAT)
    b = CC.rest_on(a, b, 1.0, direction=(1.0, 0.0, 0.0))  # the patch sits on A's +x side, around y = 64 - 1.3
    use(cq, a, b)
    got = cq.query_contacts(0, 1, CC.margins(a)[1])
    assert R.same_bits(got, reference(a, b, CC.margins(a)[1])) == []
    y = got["cell_a"][:, 1]
    assert got["contacts"] > 50 and (y < 64).any() and (y >= 64).any()  # lanes of both runs of a row


# -- 4. nothing else moves -----------------------------------------------------------------------------------------------------------------
def test_the_slots_the_history_and_the_render_state_stay_as_they_were(cq):
    a, b = CC.CASES["texel16_b"]()
    sc = use(cq, a, b)
    p = v.default_params(160, 90, float(sc.Objects[0].Volume.CellSize), v.march_budget(4, 255))
    cq.ResizeRenderOutput(p.width, p.height)
    cq.params_override = p
    cq.SetRendererMode(p.mode)
    cq.enable_history(0, 8, 1 << 24)
    before = cq.Render()
    state = (cq.last_timing(), cq.timing_history(8), cq.launch_history(8), cq.last_kernel_form(), cq.history_info(0), cq.wave_records(0).copy())
    bufs = [buffers(cq, 0), buffers(cq, 1)]
    for margin in (0.0, 0.05, 0.3):
        assert cq.query_contacts(0, 1, margin)["contacts"] > 0
        cq.query_contacts(1, 0, margin)
    after = (cq.last_timing(), cq.timing_history(8), cq.launch_history(8), cq.last_kernel_form(), cq.history_info(0), cq.wave_records(0))
    for x, y in zip(state[:5], after[:5]):
        assert x == y
    assert np.array_equal(state[5], after[5])
    for slot in (0, 1):
        now = buffers(cq, slot)
        for name in WHICH:
            assert np.array_equal(now[name], bufs[slot][name]), (slot, name)
    assert np.array_equal(cq.Render(), before)
    cq.enable_history(0, 0, 0)
    cq.params_override = None


def test_a_scene_set_while_frames_are_in_flight_is_honoured(cq):
    a, b = CC.CASES["spheres17_overlap1"]()
    sc = use(cq, a, b)
    p = v.default_params(160, 90, float(sc.Objects[0].Volume.CellSize), v.march_budget(4, 255))
    cq.ResizeRenderOutput(p.width, p.height)
    cq.params_override = p
    first = cq.query_contacts(0, 1)
    cq.render_begin(0, p)
    cq.render_begin(1, p)
    b.position = tuple(float(f32(x + d)) for x, d in zip(b.position, (-0.0625, 0.03125, 0.0)))
    sc.Objects[1].Position = b.position
    got = cq.query_contacts(0, 1)  # syncs: the scene set is deferred, frames are in flight
    cq.render_end(0, p, copy=False)
    cq.render_end(1, p, copy=False)
    cq.params_override = None
    assert R.same_bits(got, reference(a, b, 0.0)) == []
    assert R.same_bits(got, first) != []


def test_bad_indices_and_a_short_capacity_are_refused(cq):
    a, b = CC.CASES["spheres17_overlap1"]()
    use(cq, a, b)
    lib, ctx = cq._lib, cq._ctx
    res = _abi.vrt_contacts_result()
    INVALID = _abi.VRT_ERR_INVALID
    for i, j in ((0, 2), (2, 0), (-1, 1), (1, -1), (0, 64), (1, 1)):
        assert lib.vrt_query_contacts(ctx, i, j, 0.0, None, 0, C.byref(res)) == INVALID
    assert lib.vrt_query_contacts(ctx, 0, 1, -0.5, None, 0, C.byref(res)) == INVALID
    assert lib.vrt_query_contacts(ctx, 0, 1, 0.0, None, 0, None) == INVALID
    assert lib.vrt_query_contacts(ctx, 0, 1, 0.0, None, 0, C.byref(res)) == 0  # count only
    n = int(res.contacts)
    assert n == 21 and res.candidates == 194
    rec = np.frombuffer(bytearray(b"\xab" * (64 * n)), v.CONTACT_DTYPE)
    untouched = rec.tobytes()
    res2 = _abi.vrt_contacts_result()
    assert lib.vrt_query_contacts(ctx, 0, 1, 0.0, rec.ctypes.data_as(C.c_void_p), n - 1, C.byref(res2)) == INVALID
    assert rec.tobytes() == untouched and bytes(res2) == bytes(res)  # the result is filled, no output byte touched
    assert lib.vrt_query_contacts(ctx, 0, 1, 0.0, rec.ctypes.data_as(C.c_void_p), n, C.byref(res2)) == 0
    assert R.same_bits(v.contacts_to_dict(rec, res2), reference(a, b, 0.0)) == []


# -- 5. the C++ adaptor's demo -------------------------------------------------------------------------------------------------------------
def test_demo_prints_the_contacts_of_two_objects(tmp_path):
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    res = subprocess.run([exe, "--frames", "1", "--size", "320x180", "--contacts", "0", "1", "--out", str(tmp_path / "c.ppm")],
                         capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stderr
    (line,) = re.findall(r"^contacts 0 1: (\d+) contacts of (\d+) candidates, deepest distance (\S+)$", res.stdout, flags=re.M)
    assert int(line[0]) <= int(line[1])
    assert (int(line[0]) == 0) == (line[2] == "inf")
