"""The device against volumes this project did not produce: tests/golden/ref_held/ (the reference's own C++ through oracle/_ref/ref_probe,
see tests/test_ref_held.py).  Fixtures only: nothing here reads the reference tree or runs the probe.
  - vrt_voxelize_mesh on every fixture mesh, both formats: the fp32 download is the reference's densities and materials BIT FOR BIT
    (as the CPU twin is), the TEXEL16 slot their quantisation, and every buffer of both slots — bricks, cells, both levels of the
    empty-space table, the Cube table, the active box — is volume_ref.device_bytes of the REFERENCE-HELD field;
  - vrt_volume_upload_voxels of the records as the reference laid them out, then download, download_region and every buffer;
  - the reference-written scene.vox rendered through the C++ adaptor equals the same scene built in Python through the C-ABI;
  - the reference-held torus at resolution 5 marched by the literal restatement of the reference's shaders: the HIP frame with both
    reference flags stays within the bound of the closest existing literal case."""
import ctypes as C

import numpy as np
import pytest

import volume_ref as R
import voxelize_ref as V
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from test_ref_held import TIE_CASES, VOX_CASES, held_case
from test_volume_buffers_gpu import F32, T16, RefCache, check_slot, read, set_metric
from test_voxelize_gpu import SLOT_F32, SLOT_T16, shell_metric, slots, voxelize  # noqa: F401  (slots is a fixture)

pytestmark = pytest.mark.gpu


def held_buffers(h, fmt, case: V.Case) -> dict:
    """Every buffer of a slot that holds the REFERENCE-HELD shell in format fmt under the shell's metric (thr, thr/2)."""
    thr, step = shell_metric(case)
    return R.device_bytes(R.dense_field(h["density"], fmt), np.ascontiguousarray(h["material"]), fmt, thr, step)


@pytest.mark.parametrize("name", VOX_CASES + TIE_CASES)
def test_device_voxelizer_gives_the_reference_s_voxels_and_tables(slots, name):
    r = slots
    case, h = held_case(name)
    assert voxelize(r, SLOT_F32, case, F32) == 0
    gpu = r.download_volume(SLOT_F32, case.resolution, case.extent)
    assert np.array_equal(gpu.material_id, h["material"]), f"{name}: materials differ from the reference's"
    differ = gpu.density.view(np.uint32) != h["density"].view(np.uint32)
    assert not differ.any(), f"{name}: {int(differ.sum())} densities differ from the reference's, first at [x, z, y] = {np.argwhere(differ)[0]}"
    assert voxelize(r, SLOT_T16, case, T16) == 0
    N = gpu.N
    t16 = read(r, SLOT_T16, "dense").view(np.float32).reshape((N,) * 3)
    assert np.array_equal(t16.view(np.uint32), R.dense_field(h["density"], T16).view(np.uint32))
    for slot, fmt in ((SLOT_F32, F32), (SLOT_T16, T16)):
        check_slot(r, slot, held_buffers(h, fmt, case), f"{name} format {fmt}")


@pytest.mark.parametrize("fmt", [F32, T16])
@pytest.mark.parametrize("name", VOX_CASES)
def test_upload_of_the_reference_s_records_holds_the_reference(slots, name, fmt):
    """std::vector<VVoxel> as the reference lays it out (x*N*N + z*N + y, 8-byte records) through vrt_volume_upload_voxels: the
    download and a download_region of an off-centre box give the records back (TEXEL16: quantised), and every buffer is the
    host reference's of that field, under the default metric and under the shell's."""
    r = slots
    case, h = held_case(name)
    N = h["density"].shape[0]
    rec = np.zeros(N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
    rec["material"], rec["density"] = h["material"].reshape(-1), h["density"].reshape(-1)
    _abi.check(r._lib.vrt_set_volume_format(r._ctx, fmt), "vrt_set_volume_format")
    _abi.check(r._lib.vrt_volume_upload_voxels(r._ctx, SLOT_F32, case.resolution, case.extent, rec.ctypes.data_as(C.c_void_p)), "vrt_volume_upload_voxels")
    dense = R.dense_field(h["density"], fmt)
    got = r.download_volume(SLOT_F32, case.resolution, case.extent)
    want = got.density
    assert np.array_equal(got.material_id, h["material"])
    if fmt == F32:
        assert np.array_equal(got.density.view(np.uint32), h["density"].view(np.uint32))
    else:  # the decoded quantised field: less than one quantum (0.01: the texel truncates) from the reference's
        assert (np.abs(got.density - h["density"]) <= 0.01 + 1e-6)[np.abs(h["density"]) < 327.0].all()
    lo = (N // 3, 0, N // 2)
    hi = (N - 1, N // 2, N - 1)
    d, m = r.download_region(SLOT_F32, lo, hi)
    box = (slice(lo[0], hi[0] + 1), slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1))
    assert np.array_equal(d.view(np.uint32), want[box].view(np.uint32)) and np.array_equal(m, h["material"][box])
    ref = RefCache(dense, fmt)
    thr, step = shell_metric(case)
    for scale_k, step_k in ((1.0, 0.0), (float(thr), float(step))):
        set_metric(r, SLOT_F32, scale_k, step_k)
        check_slot(r, SLOT_F32, ref.want(h["material"], scale_k, step_k), f"{name} fmt {fmt} metric ({scale_k}, {step_k})")


def held_torus_scene():
    """BASELINE config 3's scene (workloads.config3_voxelized) around the reference-held torus at resolution 5."""
    case, h = held_case("torus_res5")
    vol = v.VVoxelVolume(case.resolution, case.extent)
    vol.density = np.ascontiguousarray(h["density"])
    vol.material_id = np.ascontiguousarray(h["material"])
    thr, step = shell_metric(case)
    vol.density_scale, vol.step_max = float(thr), float(step)
    vol.Material = v.VMaterial((0.8, 0.6, 0.2, 1.0), 0.8, 0.0)
    sc = scenes.config3_voxelized(5, 64, device_format=T16)
    sc.Objects = [v.VVoxelObject(Volume=vol.set_device_format(T16))]
    return sc


def test_hip_frame_of_the_reference_held_torus_against_its_literal_frame(renderer, oracle_lib):
    """The volume the REFERENCE's voxelizer made, marched by the literal restatement of the reference's shaders (through the octree
    test_ref_held.py pins to the reference's) and by the HIP kernels with both reference flags: the interior 'more than one 8-bit
    step' fraction stays within LITERAL_PIXEL_BOUNDS of the closest existing case, the voxelized torus in TEXEL16 at 320x180."""
    from oracle.binding import OracleScene
    from tests import ref_pixels
    from test_parity_gpu import LITERAL_PIXEL_BOUNDS, REF_FLAGS, gpu_render

    sc = held_torus_scene()
    p = v.default_params(320, 180, scenes.min_cell(sc), 255, shadow=True)
    lit, t, st = OracleScene(sc).ref_literal_render(p, threads=8)
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= REF_FLAGS
    img, _ = gpu_render(renderer, sc, q)
    m = ref_pixels.compare_rgb8(ref_pixels.quantise(img), ref_pixels.quantise(lit), t, p.height)
    print("ref_held: literal frame of the reference-held torus", m, st)
    assert m["interior_pixels"] > 1000
    assert m["gt1"] <= LITERAL_PIXEL_BOUNDS["ref_c3vox256_texel16_320x180"], m


def test_cpp_adaptor_renders_the_reference_written_scene_like_the_python_host(tmp_path):
    """tests/golden/ref_held/scene.vox — written by the reference's VSceneConverter and VSerializationManager — through the C++ adaptor
    (vrt_demo --scene: HostSerialization's reader, HipRenderer) at 64x36, against the same scene built in Python from vox_io.load_scene
    of the file plus what the demo adds around it (camera, sky, its two mirror spheres) through the C-ABI.  The comparison is the one of
    test_cpp_host_adaptor_binds_material_textures_from_a_vox_scene: 8-bit frames, fewer than 0.2 % of the pixels more than one step apart."""
    import os
    import subprocess

    from volumetricraytracer_amd import vox_io
    from test_parity_gpu import REFERENCE_DEFAULT_NORMAL_TEXEL
    from test_ref_held import HELD

    vox = os.path.join(HELD, "scene.vox")
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out = str(tmp_path / "demo.ppm")
    r = subprocess.run([exe, "--frames", "1", "--size", "64x36", "--scene", vox, "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    ppm = np.frombuffer(raw[raw.index(b"255\n") + 4:], dtype=np.uint8).reshape(36, 64, 3)

    held_scene = vox_io.load_scene(vox)
    assert len(held_scene.Objects) == 2 and len(held_scene.PointLights) == 1 and len(held_scene.SpotLights) == 1
    mat = lambda c: v.VMaterial(c, 0.1, 0.6)
    S = 256
    tint = np.array([[1, .85, .8], [.8, .85, 1], [.85, 1, .8], [1, .8, 1], [.6, .75, 1], [.55, .5, .45]], np.float32)
    g = (0.35 + 0.6 * (1.0 - (np.arange(S, dtype=np.float32) + 0.5) / S)).astype(np.float32)
    env = np.zeros((6, S, S, 4), np.uint8)
    for f in range(6):
        env[f, :, :, :3] = np.minimum(255.0, g[:, None, None] * tint[f][None, None, :] * 255.0 + 0.5).astype(np.uint8)
    env[..., 3] = 255
    sc = v.VScene(Camera=v.VCamera(Position=(300.0, 0.0, 100.0), Rotation=tuple(v.quat_from_axis_angle(v.UP, 3.14159265))),
                  DirectionalLight=held_scene.DirectionalLight, PointLights=held_scene.PointLights, SpotLights=held_scene.SpotLights,
                  Objects=list(held_scene.Objects) + [
                      v.VVoxelObject(Position=(200.0, 0.0, 100.0), Volume=v.sphere_volume(6, 100.0, 40.0, mat((1, 0, 0, 1)))),
                      v.VVoxelObject(Position=(100.0, 0.0, 200.0), Volume=v.sphere_volume(6, 100.0, 20.0, mat((0, 0, 1, 1))))],
                  EnvironmentMap=env)
    for vol in sc.volumes():
        vol.set_device_format(T16)  # the C++ adaptor's default
        vol.Material.NormalTexture = REFERENCE_DEFAULT_NORMAL_TEXEL  # what the adaptor binds to a material without a normal map
    r2 = v.VHipRenderer()
    assert r2.Start()
    try:
        r2.SetSceneToRender(sc)
        r2.ResizeRenderOutput(64, 36)
        r2.SetRendererMode(_abi.MODE_INTERP)
        r2.ReferenceViewVector = r2.ReferenceBoundaryTexels = True  # the adaptor's defaults
        img = r2.Render()
    finally:
        r2.Stop()
    py8 = (np.clip(img[..., :3], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    diff = np.abs(py8.astype(int) - ppm.astype(int))
    print("ref_held: adaptor vs python host on the reference-written scene:", int((diff > 1).sum()), "of", diff.size, "channel values more than one step apart, max", int(diff.max()))
    assert (diff > 1).mean() < 2e-3, f"{(diff > 1).sum()} pixels differ by more than one 8-bit step"
    assert (ppm[..., 0].astype(int) - ppm[..., 2] > 60).sum() > 20  # the demo's red sphere is in the frame
