"""Mesh extraction on the device (vrt_volume_extract_mesh) against the numpy reference of the contract (tests/mesh_ref.py): tolerance 0
on position and normal bits, material bytes, indices and the result record; the call's argument and capacity rules; and that it only
reads the slot — every device buffer is the same before and after."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import brush_ref as B
import fill_ref as F
import mesh_ref as MR
import redistance_ref as RR
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from test_volume_fill_gpu import EDITED, FULL, assert_same_buffers, buffers, upload_field
from test_volume_mesh import FIELDS, all_boxes, assert_same_mesh, case, isos, reference

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
    vol.density_scale = f.scale
    upload_field(r, slot, vol, f.fmt, f.stored, f.material)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", FIELDS)
def test_device_mesh_equals_the_reference(renderer, name, fmt):
    """17^3 and 33^3: every field, the whole grid and every box, three levels; the slot's buffers untouched by all of it."""
    f = case(name, int(fmt))
    upload_case(renderer, f)
    before = buffers(renderer, EDITED)
    calls = 0
    for box, (lo, hi) in all_boxes(name, f.N).items():
        for iso in isos(name):
            got = renderer.extract_mesh(EDITED, iso, lo, hi)
            assert_same_mesh(got, reference(name, int(fmt), iso, box), f"{name}, format {fmt}, iso {iso}, box {box}")
            calls += 1
    assert_same_buffers(buffers(renderer, EDITED), before, f"{name}, format {fmt}: after {calls} extractions")


@functools.lru_cache(maxsize=None)
def sphere_129():
    """A sphere of 40.4 cells on 129^3 (resolution 7): a row has 128 cells, two runs of 64 cells, and the surface crosses the run
    boundary at y = 64 on either side of the centre."""
    cell, _ = B.units(129, 100.0, 1.0)
    density = RR.sphere_field(129, (64.3, 63.8, 64.1), 40.4, float(cell))
    material = F.hand_made_material(density)
    for a in (density, material):
        a.setflags(write=False)
    return density, material


@pytest.mark.parametrize("box", [None, ((21, 3, 40), (100, 90, 127))])
def test_a_sphere_on_129(renderer, box):
    """The off-centre box starts its rows at y = 3, so its runs (y = 3..66, 67..89) do not line up with the whole grid's."""
    density, material = sphere_129()
    vol = v.VVoxelVolume(7, 100.0)
    upload_field(renderer, EDITED, vol, _abi.FORMAT_F32, density, material)
    lo, hi = box if box else (None, None)
    want = MR.extract(density, material, R.F32, 0.0, 100.0, lo, hi)
    got = renderer.extract_mesh(EDITED, 0.0, lo, hi)
    assert_same_mesh(got, want, f"sphere on 129^3, box {box}")
    assert want[4]["vertices"] > (30000 if box is None else 10000)
    if box is None:
        most, unpaired, E = MR.edge_census(got[3], len(got[0]))
        assert most == 1 and len(unpaired) == 0 and len(got[0]) - E + len(got[3]) == 2


def raw_call(r, slot, iso=0.0, o=None, s=None, pos=None, nrm=None, mat=None, vcap=0, idx=None, icap=0, ctx=True):
    res = _abi.vrt_mesh_result()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = r._lib.vrt_volume_extract_mesh(r._ctx if ctx else None, slot, iso, o, s, p(pos), p(nrm), p(mat), vcap, p(idx), icap, C.byref(res))
    return rc, (tuple(res.lo), tuple(res.hi), int(res.vertices), int(res.quads))


def sentinels(V, Q):
    return (np.full((V, 3), 7.5, np.float32), np.full((V, 3), -3.25, np.float32), np.full(V, 0xA5, np.uint8), np.full(6 * Q, 0xDEADBEEF, np.uint32))


def untouched(pos, nrm, mat, idx):
    return bool((pos == 7.5).all() and (nrm == -3.25).all() and (mat == 0xA5).all() and (idx == 0xDEADBEEF).all())


def test_counting_capacities_and_null_arrays(renderer):
    f = case("small sphere", R.TEXEL16)
    upload_case(renderer, f)
    want = reference("small sphere", R.TEXEL16, 0.0, "whole grid")
    V, Q = want[4]["vertices"], want[4]["quads"]
    record = (want[4]["lo"], want[4]["hi"], V, Q)
    rc, counted = raw_call(renderer, EDITED)
    assert rc == _abi.VRT_OK and counted == record
    # the full call reports the same record
    pos, nrm, mat, idx = sentinels(V + 3, Q + 2)  # room to spare: nothing beyond the mesh is written
    rc, full = raw_call(renderer, EDITED, pos=pos, nrm=nrm, mat=mat, vcap=V + 3, idx=idx, icap=6 * Q + 12)
    assert rc == _abi.VRT_OK and full == record
    assert_same_mesh((pos[:V], nrm[:V], mat[:V], idx[:6 * Q].reshape(-1, 3), want[4]), want, "full call")
    assert untouched(pos[V:], nrm[V:], mat[V:], idx[6 * Q:])
    # a capacity one short on either side: VRT_ERR_INVALID with the counts, nothing written
    for vcap, icap in ((V - 1, 6 * Q), (V, 6 * Q - 1)):
        pos, nrm, mat, idx = sentinels(V, Q)
        rc, short = raw_call(renderer, EDITED, pos=pos, nrm=nrm, mat=mat, vcap=vcap, idx=idx, icap=icap)
        assert rc == _abi.VRT_ERR_INVALID and short == record and untouched(pos, nrm, mat, idx), (vcap, icap)
    # a short index capacity refuses even when only vertex arrays were asked for, and the other way round
    pos, nrm, mat, idx = sentinels(V, Q)
    assert raw_call(renderer, EDITED, pos=pos, vcap=V, icap=0)[0] == _abi.VRT_ERR_INVALID and untouched(pos, nrm, mat, idx)
    # each NULL array alone is skipped, the others are written
    for skip in range(4):
        arrays = list(sentinels(V, Q))
        given = [None if i == skip else a for i, a in enumerate(arrays)]
        rc, rec = raw_call(renderer, EDITED, pos=given[0], nrm=given[1], mat=given[2], vcap=V, idx=given[3], icap=6 * Q)
        assert rc == _abi.VRT_OK and rec == record
        got = [arrays[0], arrays[1], arrays[2], arrays[3].reshape(-1, 3)]
        for i in range(4):
            if i == skip:
                assert np.array_equal(arrays[i], sentinels(V, Q)[i]), skip
            elif i < 2:
                assert np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32)), (skip, i)
            else:
                assert np.array_equal(got[i], want[i]), (skip, i)


def test_refused_calls_leave_the_outputs_alone(renderer):
    f = case("small sphere", R.F32)
    upload_case(renderer, f)
    before = buffers(renderer, EDITED)
    V, Q = 2000, 2000
    pos, nrm, mat, idx = sentinels(V, Q)
    out = dict(pos=pos, nrm=nrm, mat=mat, vcap=V, idx=idx, icap=6 * Q)
    box = lambda *a: (C.c_int * 3)(*a)
    assert raw_call(renderer, 7, **out)[0] == _abi.VRT_ERR_SLOT
    assert raw_call(renderer, _abi.VRT_MAX_VOLUMES, **out)[0] == _abi.VRT_ERR_SLOT
    assert raw_call(renderer, -1, **out)[0] == _abi.VRT_ERR_SLOT
    assert raw_call(renderer, EDITED, ctx=False, **out)[0] == _abi.VRT_ERR_INVALID
    for iso in (float("nan"), float("inf"), -float("inf")):
        assert raw_call(renderer, EDITED, iso, **out)[0] == _abi.VRT_ERR_INVALID, iso
    assert raw_call(renderer, EDITED, 0.0, box(0, 0, 0), None, **out)[0] == _abi.VRT_ERR_INVALID
    assert raw_call(renderer, EDITED, 0.0, None, box(2, 2, 2), **out)[0] == _abi.VRT_ERR_INVALID
    for o, s in (((-1, 0, 0), (2, 2, 2)), ((0, 0, 0), (18, 1, 1)), ((16, 16, 16), (1, 2, 1)), ((3, 3, 3), (0, 1, 1))):
        assert raw_call(renderer, EDITED, 0.0, box(*o), box(*s), **out)[0] == _abi.VRT_ERR_INVALID, (o, s)
    assert untouched(pos, nrm, mat, idx)
    assert_same_buffers(buffers(renderer, EDITED), before, "after refused calls")
    assert renderer._lib.vrt_volume_extract_mesh(renderer._ctx, EDITED, 0.0, None, None, None, None, None, 0, None, 0, None) == _abi.VRT_OK


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_mesh_of_a_sculpted_volume(renderer, fmt):
    """The editing chain of test_fill_redistance_carve_redistance — fill, redistance FROM_OUTSIDE, a smooth SUBTRACT dab — and then the
    mesh, against the reference's mesh of the reference's edited field."""
    vol = copy.copy(scenes.voxelized_torus(5)).set_device_format(fmt)
    stored = R.dense_field(np.array(vol.density, np.float32), int(fmt))
    material = np.array(vol.material_id, np.uint8)
    _, unit = B.units(vol.N, vol.VolumeExtends, vol.density_scale)
    upload_field(renderer, EDITED, vol, fmt, stored, material)
    renderer.fill_enclosed(EDITED, None, 1.0, 1)
    want_d, want_m, _ = F.fill(stored, material, int(fmt), 1.0, 1)
    renderer.redistance(EDITED, None, 3, RR.OUTSIDE)
    want_d, _ = RR.redistance(want_d, int(fmt), 3, RR.OUTSIDE, unit)
    rec = v.sphere_brush(_abi.BRUSH_SUBTRACT, (24.6, 16.0, 16.0), 3.0, 1.5, 3.0, 0)
    dab = renderer.apply_brushes(EDITED, None, [rec])
    want_d, want_m = np.array(want_d), np.array(want_m)
    assert dab == B.apply(want_d, want_m, int(fmt), [rec], vol.VolumeExtends, vol.density_scale) and dab["written"] > 50
    before = buffers(renderer, EDITED)
    assert_same_buffers(before, R.device_bytes(want_d, want_m, int(fmt), vol.density_scale, vol.step_max), "the edited slot")
    want = MR.extract(want_d, want_m, int(fmt), 0.0, vol.VolumeExtends)
    got = renderer.extract_mesh(EDITED)
    assert_same_mesh(got, want, f"format {fmt}: sculpted torus")
    assert want[4]["vertices"] > 1500
    most, unpaired, _ = MR.edge_census(got[3], len(got[0]))
    assert most == 1 and len(unpaired) == 0  # a closed surface with a dent
    assert_same_buffers(buffers(renderer, EDITED), before, "after the extraction")


def test_a_context_over_two_devices_gives_the_same_mesh():
    f = case("filled torus 5", R.TEXEL16)
    want = reference("filled torus 5", R.TEXEL16, 0.0, "whole grid")
    with v.VHipRenderer(devices=(0, 0)) as r:
        upload_case(r, f)
        got = r.extract_mesh(EDITED)
    assert_same_mesh(got, want, "two devices")


def test_vox2gltf_writes_the_same_bytes_with_and_without_the_device(tmp_path):
    import os
    import subprocess
    from test_volume_mesh import VOX2GLTF, sphere_scene
    sphere_scene(str(tmp_path / "scene.vox"))
    files = {}
    for name, extra in (("cpu", []), ("gpu", ["--gpu"])):
        for suffix in (".gltf", ".glb"):
            out = str(tmp_path / (name + suffix))
            r = subprocess.run([VOX2GLTF] + extra + ["--iso", "0.5", "--out", out, str(tmp_path / "scene.vox")], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            assert int(r.stdout.split(" vertices")[0].split()[-1]) not in (0, 2046), r.stdout  # iso 0.5 is not the surface at 0
            assert ("device extraction" in r.stdout) == (name == "gpu")
            files[(name, suffix)] = open(out, "rb").read()
        files[(name, ".bin")] = open(str(tmp_path / (name + ".bin")), "rb").read()
    for suffix in (".glb", ".bin"):
        assert files[("cpu", suffix)] == files[("gpu", suffix)] and len(files[("cpu", suffix)]) > 50000, suffix
    # the two manifests differ only in the name of their buffer file
    assert files[("cpu", ".gltf")].replace(b"cpu.bin", b"gpu.bin") == files[("gpu", ".gltf")]


def test_cpp_adaptor_writes_the_sculpted_model(tmp_path):
    """vrt_demo --solid --edit-brush 12 --edit-device --mesh-out: the red sphere (radius 40 of extent 100 on 65^3: 12.8 cells), filled and
    carved by four dabs of 12 cells, through VHipRenderer::ExtractMesh and the glTF writer; the importer loads the file."""
    import os
    import subprocess
    from volumetricraytracer_amd import voxelizer as vx
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out, mesh = str(tmp_path / "frame.ppm"), str(tmp_path / "sculpted.glb")
    r = subprocess.run([exe, "--solid", "--frames", "4", "--size", "160x90", "--edit-brush", "12", "--edit-device", "--out", out, "--mesh-out", mesh],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("mesh:")]
    assert len(lines) == 1 and "device brushes" in r.stdout, r.stdout
    V, T = int(lines[0].split()[1]), int(lines[0].split()[3])
    # a sphere of 12.8 cells has some 4 pi r^2 = 2000 cells of surface, surface nets make about 1.5 vertices per unit of area, and the
    # dabs add their own walls: thousands, far from the 64^3 = 262144 cells of the grid; a closed surface has T near 2 V
    assert 2000 < V < 20000 and abs(T - 2 * V) < 200, lines[0]
    name, pos, idx = vx.import_gltf_mesh(mesh)
    assert name == "Object0_6" and len(pos) == V and idx.size == 3 * T and int(idx.max()) == V - 1
