"""vrt_voxelize_mesh — the producer of the benchmark's own volume — against the independent float64 reference of
tests/voxelize_ref.py and, bit for bit, against its CPU twin, at the edges the three closed, centred meshes of test_parity_gpu.py never
reach: triangles cut, thinned to one voxel or left out by the clip, resolutions 0-2 and 8-9, an extent whose background lies below far
densities, needles, sub-cell and duplicated triangles under atomicMin contention, damaged vertices, an empty mesh, a re-voxelized slot,
two devices and refused calls.  Each comparison with the reference prints its worst error in units of (N-1) * 2^-23 (the tolerance
is 4): profiles/voxelize_reference.txt."""
import ctypes as C

import numpy as np
import pytest

import volume_ref as R
import voxelize_ref as V
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from test_volume_buffers_gpu import F32, T16, WHICH, check_slot, read, set_metric
from test_voxelize_ref import ILL, check_ill, check_well, cpu_twin, well_cases

pytestmark = pytest.mark.gpu
SLOT_F32, SLOT_T16, SLOT_OLD = 12, 13, 14
WELL = well_cases(resolutions=(0, 1, 2, 4, 6))


@pytest.fixture
def slots(renderer):
    """Three slots of the session's renderer that start unused, hold F32 uploads again afterwards and are freed."""
    def free():
        for slot in (SLOT_F32, SLOT_T16, SLOT_OLD):
            renderer._uploaded.pop(slot, None)
            renderer._lib.vrt_volume_free(renderer._ctx, slot)  # VRT_ERR_SLOT when unused
        _abi.check(renderer._lib.vrt_set_volume_format(renderer._ctx, F32), "vrt_set_volume_format")
    free()
    yield renderer
    free()


def voxelize(r, slot, case: V.Case, fmt=F32):
    _abi.check(r._lib.vrt_set_volume_format(r._ctx, fmt), "vrt_set_volume_format")
    return r.voxelize_mesh(slot, case.positions, case.indices, case.resolution, case.extent)


def shell_metric(case: V.Case):
    N, cell, thr = V.grid(case.resolution, case.extent)
    return np.float32(thr), np.float32(0.5) * np.float32(thr)


def shell_buffers(f32_field, fmt, case: V.Case) -> dict:
    """Every buffer of a slot that holds the shell f32_field in format fmt under the metric (thr, thr/2)."""
    thr, step = shell_metric(case)
    return R.device_bytes(R.dense_field(f32_field, fmt), (f32_field <= 0).astype(np.uint8), fmt, thr, step)


def assert_same_bits(gpu, cpu, what):
    assert np.array_equal(gpu.density.view(np.uint32), cpu.density.view(np.uint32)), f"{what}: densities differ from the CPU twin"
    assert np.array_equal(gpu.material_id, cpu.material_id), f"{what}: materials differ from the CPU twin"


# ---- a. against the reference, both formats; b. against the CPU twin ------------------------------------------------------------

@pytest.mark.parametrize("name", list(WELL))
def test_device_matches_the_reference_and_the_cpu_twin(slots, capfd, name):
    """Well-conditioned triangles, many of them cut by the clip: the whole grid within the derived tolerance of the float64
    reference, the background exact, materials, the skipped count; the same bits as the CPU converter; every buffer of the slot, in
    both formats, is the one of the downloaded field under the shell's metric (thr, thr/2), the TEXEL16 one its quantisation."""
    r, case = slots, WELL[name]()
    cpu, skipped = cpu_twin(case, capfd)
    assert skipped == 0
    assert voxelize(r, SLOT_F32, case, F32) == case.skipped == 0
    gpu = r.download_volume(SLOT_F32, case.resolution, case.extent)
    check_well(case, gpu.density, gpu.material_id, "device")
    assert_same_bits(gpu, cpu, name)
    assert voxelize(r, SLOT_T16, case, T16) == 0
    N = gpu.N
    dense = read(r, SLOT_F32, "dense").view(np.float32).reshape((N,) * 3)
    assert np.array_equal(dense.view(np.uint32), gpu.density.view(np.uint32))
    for slot, fmt in ((SLOT_F32, F32), (SLOT_T16, T16)):
        check_slot(r, slot, shell_buffers(dense, fmt, case), f"{name} format {fmt}")
    # the TEXEL16 download decodes the quantised field: the materials are those of the fp32 run
    assert np.array_equal(r.download_volume(SLOT_T16, case.resolution, case.extent).material_id, gpu.material_id)


@pytest.mark.parametrize("name", list(ILL))
def test_device_matches_the_cpu_twin_on_ill_conditioned_and_damaged_input(slots, capfd, name):
    """Sub-cell triangles, needles (every 7th exactly degenerate), a torus with duplicated faces, half of each through a face of the
    volume, and a mesh with NaN, infinite and huge vertices, an index out of range and dangling indices: densities, materials and the
    skipped count are the CPU converter's, bit for bit (an integer atomicMin on keys against a sequential `<`), and hold what any
    input must."""
    r, case = slots, ILL[name]()
    assert voxelize(r, SLOT_F32, case, F32) == case.skipped
    gpu = r.download_volume(SLOT_F32, case.resolution, case.extent)
    cpu, skipped = cpu_twin(case, capfd)
    assert skipped == case.skipped
    assert_same_bits(gpu, cpu, name)
    check_ill(case, gpu.density, gpu.material_id, "device")
    check_slot(r, SLOT_F32, shell_buffers(gpu.density, F32, case), name)


# ---- c. large grids -----------------------------------------------------------------------------------------------------------------

def check_sample(case, density, material, at, who):
    """The voxels `at` of a dense field against the reference."""
    N = V.grid(case.resolution, case.extent)[0]
    ref = V.reference(case.triangles(), case.resolution, case.extent, at)
    assert ref.ambiguous == 0
    got = density[at[:, 0], at[:, 2], at[:, 1]]
    err = V.scaled_error(N, got, ref.density)
    print(f"voxelize_reference: {case.name:28s} {who:6s} worst scaled error {err:.3f} on {len(at)} voxels")
    assert (np.abs(got.astype(np.float64) - ref.density) <= V.tol(N, ref.density)).all(), (case.name, err)
    assert (got[~ref.covered] == np.float32(2.0 * case.extent)).all()
    check = np.abs(ref.density) > V.tol(N, ref.density)
    assert (~check).sum() <= V.LEFT_OUT_SHARE * check.size
    assert np.array_equal(material[at[:, 0], at[:, 2], at[:, 1]][check], ref.material[check])
    return ref


def test_device_at_257_matches_the_cpu_twin_and_the_reference(slots, capfd):
    """N = 257: small triangles in the far corner (indices >= 232) and through the three far faces, and one triangle whose box is the
    whole grid — 17 million voxels walked by one workgroup.  Bit for bit the CPU converter; the far corner, the two outermost layers of
    every face and a seeded sample against the reference."""
    r, case = slots, V.large_mesh(8, whole=True)
    N = 257
    lo, hi, _ = V.boxes(case.triangles(), 8, case.extent)
    assert (lo[:24] >= 232).all() and (lo[-1] == 0).all() and (hi[-1] == N - 1).all()
    assert voxelize(r, SLOT_F32, case) == 0
    gpu = r.download_volume(SLOT_F32, 8, case.extent)
    cpu, skipped = cpu_twin(case, capfd)
    assert skipped == 0
    assert_same_bits(gpu, cpu, case.name)
    at = V.large_sample(8)
    assert len(at) >= 300000
    ref = check_sample(case, gpu.density, gpu.material_id, at, "device")
    assert ref.covered.all() and (gpu.density[N - 24:, N - 24:, N - 24:] <= 0).sum() > 100
    assert np.array_equal(gpu.material_id == 1, gpu.density <= 0)


def test_device_at_513_matches_the_reference():
    """N = 513, which the CPU converter refuses: the mesh of the 257 test in cells of this grid, its whole-grid triangle replaced by
    one whose box is the upper half (some 70 million voxels for one workgroup).  The far corner, the face layers
    and a sample against the reference; every voxel outside all of the reference's boxes holds the background."""
    case = V.large_mesh(9, whole=False)
    N = 513
    tri = case.triangles()
    lo, hi, amb = V.boxes(tri, 9, case.extent)
    assert amb == 0 and (lo[:24] >= N - 25).all()
    assert np.prod(hi[-1] - lo[-1] + 1, dtype=np.int64) > N ** 3 // 2
    at = V.large_sample(9)
    with v.VHipRenderer() as r:
        assert voxelize(r, SLOT_F32, case) == 0
        density = read(r, SLOT_F32, "dense").view(np.float32).reshape((N,) * 3)
        material = read(r, SLOT_F32, "material").reshape((N,) * 3)
        _abi.check(r._lib.vrt_volume_free(r._ctx, SLOT_F32), "vrt_volume_free")
    check_sample(case, density, material, at, "device")
    outside = ~V.in_boxes(lo, hi, N)
    assert outside.sum() > N ** 3 // 4
    assert (density[outside] == np.float32(2.0 * case.extent)).all() and not material[outside].any()
    del outside
    assert np.array_equal(material == 1, density <= 0)


# ---- d. lifecycle and arguments -------------------------------------------------------------------------------------------------------

def all_buffers(r, slot, device=0):
    return {name: read(r, slot, name, device) for name in WHICH}


def test_empty_index_list_gives_the_background_and_a_frame_of_sky():
    """No triangle: the fill and the finish kernels run without the voxelizing one between them."""
    from test_parity_gpu import gpu_render

    res, extent = 4, 50.0
    with v.VHipRenderer() as r:
        _empty_mesh(r, res, extent, gpu_render)


def _empty_mesh(r, res, extent, gpu_render):
    pos = np.zeros((3, 3), np.float32)
    for positions, indices in ((pos, np.zeros(0, np.uint32)), (np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)), (pos, np.array([0, 1], np.uint32))):
        assert r.voxelize_mesh(SLOT_F32, positions, indices, res, extent) == 0
        got = r.download_volume(SLOT_F32, res, extent)
        assert (got.density == np.float32(100.0)).all() and not got.material_id.any()
    # a frame of it is the frame of no object at all
    blank = v.VVoxelVolume(res, extent)
    blank.density = np.full((17,) * 3, 100.0, np.float32)
    blank.material_id = np.zeros((17,) * 3, np.uint8)
    sc = v.VScene(Camera=v.look_minus_x_camera(150.0), DirectionalLight=v.demo_light(), Objects=[v.VVoxelObject(Volume=blank)],
                  EnvironmentMap=v.procedural_skybox(16))
    prm = v.default_params(96, 54, blank.GetCellSize(), 255, shadow=True)
    sky, _ = gpu_render(r, v.VScene(Camera=sc.Camera, DirectionalLight=sc.DirectionalLight, Objects=[], EnvironmentMap=sc.EnvironmentMap), prm)
    gpu_render(r, sc, prm)
    abi_scene = sc.to_abi()
    abi_scene.instances[0].volume_slot = SLOT_F32
    _abi.check(r._lib.vrt_scene_set(r._ctx, C.byref(abi_scene)), "vrt_scene_set")
    got = np.empty_like(sky)
    _abi.check(r._lib.vrt_render(r._ctx, C.byref(prm), got.ctypes.data_as(C.c_void_p)), "vrt_render")
    assert r.last_timing()["hits"] == 0
    assert np.array_equal(got, sky)


@pytest.mark.parametrize("old_fmt,new_fmt", [(T16, F32), (F32, T16)])
def test_voxelizing_into_a_used_slot_equals_a_fresh_slot(slots, old_fmt, new_fmt):
    """The slot holds a volume of another resolution, the other format and a hand-set metric: afterwards every buffer is the one of a
    slot that was never used, and of the reference."""
    from test_volume_buffers_gpu import sample_volume, upload

    r, case = slots, V.clipped_soup(4, 40, 1.4)
    old = sample_volume(5)
    upload(r, SLOT_OLD, old, old_fmt, "float")
    set_metric(r, SLOT_OLD, 0.37, 2.0 * float(old.CellSize))
    assert voxelize(r, SLOT_OLD, case, new_fmt) == 0
    assert voxelize(r, SLOT_F32, case, new_fmt) == 0
    fresh = all_buffers(r, SLOT_F32)
    for name, have in all_buffers(r, SLOT_OLD).items():
        assert np.array_equal(have, fresh[name]), f"re-voxelized slot, {old_fmt} -> {new_fmt}: buffer {name} differs from a fresh slot's"
    assert voxelize(r, SLOT_T16, case, F32) == 0  # the fp32 field the buffers of either format derive from (pinned elsewhere)
    dense = read(r, SLOT_T16, "dense").view(np.float32).reshape((17,) * 3)
    check_slot(r, SLOT_OLD, shell_buffers(dense, new_fmt, case), "re-voxelized slot against the reference")
    # and once more into the same slot, now smaller: resolution 2 after 4
    small = V.clipped_soup(2, 4, 1.4)
    assert voxelize(r, SLOT_OLD, small, new_fmt) == 0
    assert voxelize(r, SLOT_T16, small, new_fmt) == 0
    fresh = all_buffers(r, SLOT_T16)
    for name, have in all_buffers(r, SLOT_OLD).items():
        assert np.array_equal(have, fresh[name]), f"re-voxelized slot, resolution 4 -> 2: buffer {name}"


def test_two_devices_hold_the_same_bytes():
    case = V.clipped_soup(4, 40, 1.4)
    with v.VHipRenderer(devices=(0, 0)) as r:
        for slot, fmt in ((SLOT_F32, F32), (SLOT_T16, T16)):
            assert voxelize(r, slot, case, fmt) == 0
            first, second = all_buffers(r, slot, 0), all_buffers(r, slot, 1)
            for name in WHICH:
                assert first[name].size == second[name].size and np.array_equal(first[name], second[name]), f"format {fmt} buffer {name}"
        dense = read(r, SLOT_F32, "dense").view(np.float32).reshape((17,) * 3)
        check_well(case, dense, read(r, SLOT_F32, "material", 1).reshape((17,) * 3), "dev 1")
        for slot, fmt in ((SLOT_F32, F32), (SLOT_T16, T16)):
            check_slot(r, slot, shell_buffers(dense, fmt, case), f"two devices format {fmt}", devices=(0, 1))


def test_refused_calls_return_their_codes_and_leave_the_slot_alone(slots):
    r, case = slots, V.clipped_soup(4, 40, 1.4)
    assert voxelize(r, SLOT_F32, case) == 0
    before = all_buffers(r, SLOT_F32)
    pos = np.ascontiguousarray(case.positions)
    idx = np.ascontiguousarray(case.indices)
    P, I = pos.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)
    skipped = C.c_size_t(77)

    def call(slot=SLOT_F32, resolution=4, extent=50.0, positions=P, n_vertices=len(pos), indices=I, n_indices=len(idx), ctx=r._ctx):
        return r._lib.vrt_voxelize_mesh(ctx, slot, resolution, extent, positions, n_vertices, indices, n_indices, C.byref(skipped))

    assert call(positions=None) == _abi.VRT_ERR_INVALID          # null positions with vertices
    assert call(indices=None) == _abi.VRT_ERR_INVALID
    assert call(ctx=None) == _abi.VRT_ERR_INVALID
    assert call(slot=-1) == _abi.VRT_ERR_SLOT
    assert call(slot=_abi.VRT_MAX_VOLUMES) == _abi.VRT_ERR_SLOT
    assert call(resolution=_abi.VRT_MAX_RESOLUTION + 1) == _abi.VRT_ERR_INVALID
    for extent in (0.0, -50.0, float("nan")):
        assert call(extent=extent) == _abi.VRT_ERR_INVALID, extent
    assert skipped.value == 77                                   # nothing was counted
    after = all_buffers(r, SLOT_F32)
    for name in WHICH:
        assert np.array_equal(before[name], after[name]), f"a refused call changed buffer {name}"
    # null arrays are fine when they are empty
    assert r._lib.vrt_voxelize_mesh(r._ctx, SLOT_T16, 2, 50.0, None, 0, None, 0, None) == _abi.VRT_OK
    assert (r.download_volume(SLOT_T16, 2, 50.0).density == np.float32(100.0)).all()
