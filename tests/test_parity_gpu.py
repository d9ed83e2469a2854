"""GPU parity: the HIP path through the C-ABI against the CPU oracle (and the frozen golden
images) on identical inputs.  Tolerance: 1e-4 per channel (BASELINE.json north_star); in
practice the march is bit-identical and only powf differs in the last ulp.  Ray / step
counters must agree exactly (integers)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from volumetricraytracer_amd import workloads as scenes
import volumetricraytracer_amd as v
from oracle.binding import OracleScene
from volumetricraytracer_amd import _abi

pytestmark = pytest.mark.gpu
TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
STAT_KEYS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits", "exhausted_rays")


def gpu_render(r, sc, p):
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)
    img = r.Render()
    return img, r.last_timing()


def assert_parity(r, sc, p, check_stats=True):
    img, t = gpu_render(r, sc, p)
    ref, st = OracleScene(sc).render(p, threads=8)
    err = np.abs(img - ref)
    assert not np.isnan(img).any()
    assert err.max() <= TOL, f"max abs err {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
    if check_stats:
        assert {k: t[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}
    return img, t


@pytest.mark.parametrize("path", [_abi.PATH_DENSE, _abi.PATH_BRICK, _abi.PATH_BRICK_LDS, _abi.PATH_AUTO])
def test_config2_sphere_parity(renderer, oracle_lib, path):
    sc = scenes.config2_sphere()
    p = v.default_params(320, 180, scenes.min_cell(sc), 128, path=path)
    assert_parity(renderer, sc, p)


def test_config2_full_size(renderer, oracle_lib):
    sc = scenes.config2_sphere()
    p = v.default_params(1280, 720, scenes.min_cell(sc), 128)
    img, t = assert_parity(renderer, sc, p)
    assert t["primary_rays"] == 1280 * 720


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("path", [_abi.PATH_DENSE, _abi.PATH_BRICK, _abi.PATH_BRICK_LDS])
def test_config3_torus_parity(renderer, oracle_lib, shadow, path):
    sc = scenes.config3_torus(7, 64)
    p = v.default_params(480, 270, scenes.min_cell(sc), 255, shadow=shadow, path=path)
    assert_parity(renderer, sc, p)


@pytest.mark.parametrize("path", [_abi.PATH_BRICK, _abi.PATH_BRICK_LDS])
def test_config3_at_256_cubed(renderer, oracle_lib, path):
    sc = scenes.config3_torus(8, 256)
    p = v.default_params(640, 360, scenes.min_cell(sc), 255, shadow=True, path=path)
    assert_parity(renderer, sc, p)


@pytest.mark.parametrize("distinct", [False, True])
def test_config5_instances_bvh_parity(renderer, oracle_lib, distinct):
    sc = scenes.config5_instances(6, 32, distinct_volumes=distinct)
    p = v.default_params(480, 270, scenes.min_cell(sc), 255, shadow=True)
    # the BVH visits instances in a different order than the oracle's brute-force loop, so the
    # per-instance march budget is spent differently: images must agree, step counters need not
    img, t = assert_parity(renderer, sc, p, check_stats=False)
    ref, st = OracleScene(sc).render(p, threads=8)
    assert t["hits"] == st["hits"] and t["shadow_rays"] == st["shadow_rays"]


def test_unlit_mode_and_modes_without_textures_agree(renderer, oracle_lib):
    sc = scenes.config3_torus(6, 16)
    cell = scenes.min_cell(sc)
    lit = {}
    for mode in (_abi.MODE_INTERP, _abi.MODE_INTERP_NOTEX, _abi.MODE_INTERP_UNLIT, _abi.MODE_INTERP_NOTEX_UNLIT):
        p = v.default_params(192, 108, cell, 255, shadow=True, mode=mode)
        lit[mode], _ = assert_parity(renderer, sc, p)
    assert np.array_equal(lit[_abi.MODE_INTERP], lit[_abi.MODE_INTERP_NOTEX])
    assert np.array_equal(lit[_abi.MODE_INTERP_UNLIT], lit[_abi.MODE_INTERP_NOTEX_UNLIT])


@pytest.mark.parametrize("scene_name", ["sphere", "torus_shell", "instances", "mirror_lights"])
def test_cube_modes_parity(renderer, oracle_lib, scene_name):
    """Cube render modes (SH/Raytracing_Cube*.hlsl): exact voxel-grid traversal with the brick distance table.
    Same bar as the interpolated modes: <= 1e-4 per channel, node-visit counters exact."""
    if scene_name == "sphere":
        sc, w, h = scenes.config2_sphere(), 320, 180
    elif scene_name == "torus_shell":
        sc, w, h = scenes.config3_voxelized(6, 16), 320, 180
    elif scene_name == "instances":
        sc, w, h = scenes.config5_instances(5, 16), 320, 180
    else:
        sc, w, h = scenes.full_closest_hit_scene(), 240, 136
    cell = scenes.min_cell(sc)
    imgs = {}
    for mode in (_abi.MODE_CUBE, _abi.MODE_CUBE_NOTEX, _abi.MODE_CUBE_UNLIT, _abi.MODE_CUBE_NOTEX_UNLIT):
        p = v.default_params(w, h, cell, 255, shadow=True, mode=mode)
        p.max_bounces = 2
        imgs[mode], t = assert_parity(renderer, sc, p, check_stats=(scene_name != "instances" and scene_name != "mirror_lights"))
        assert t["hits"] > 0
    assert np.array_equal(imgs[_abi.MODE_CUBE], imgs[_abi.MODE_CUBE_NOTEX])
    assert np.array_equal(imgs[_abi.MODE_CUBE_UNLIT], imgs[_abi.MODE_CUBE_NOTEX_UNLIT])
    # the blocky image differs from the interpolated one (the modes really are different paths)
    p = v.default_params(w, h, cell, 255, shadow=True, mode=_abi.MODE_INTERP_NOTEX)
    p.max_bounces = 2
    smooth, _ = gpu_render(renderer, sc, p)
    assert np.abs(smooth - imgs[_abi.MODE_CUBE_NOTEX]).max() > 0.05


def test_textured_modes_parity(oracle_lib):
    """Tri-planar albedo / RM / normal textures (SH/Include/Textures.hlsli) in the four textured render modes, with
    point + spot lights and mirror bounces; the NoTex modes of the same scene ignore them."""
    sc = scenes.textured_scene()
    cell = scenes.min_cell(sc)
    r = v.VHipRenderer()
    assert r.Start()
    try:
        imgs = {}
        for mode in (_abi.MODE_INTERP, _abi.MODE_INTERP_UNLIT, _abi.MODE_CUBE, _abi.MODE_CUBE_UNLIT, _abi.MODE_INTERP_NOTEX):
            p = v.default_params(240, 136, cell, 255, shadow=True, mode=mode)
            p.max_bounces = 2
            imgs[mode], t = assert_parity(r, sc, p, check_stats=False)
            ref, st = OracleScene(sc).render(p, threads=8)
            assert {k: t[k] for k in ("primary_rays", "shadow_rays", "bounce_rays", "hits")} == \
                   {k: st[k] for k in ("primary_rays", "shadow_rays", "bounce_rays", "hits")}
        plain = scenes.full_closest_hit_scene()
        p = v.default_params(240, 136, cell, 255, shadow=True, mode=_abi.MODE_INTERP_NOTEX)
        p.max_bounces = 2
        notex, _ = gpu_render(r, plain, p)
        assert np.array_equal(notex, imgs[_abi.MODE_INTERP_NOTEX])               # NoTex ignores the textures
        assert np.abs(imgs[_abi.MODE_INTERP] - notex).max() > 0.1                 # the textured mode does not
        # a material without textures renders the same in the textured and the NoTex mode
        p.mode = _abi.MODE_INTERP
        same, _ = gpu_render(r, plain, p)
        assert np.array_equal(same, notex)
    finally:
        r.Stop()


def test_swapping_a_material_texture_reaches_the_device(oracle_lib):
    """a new image assigned to vol.Material (the voxels untouched, so the volume is not re-uploaded) must be
    uploaded and bound at the next SyncWithScene, the old image's id freed only afterwards, and an id that is handed out again
    must never be what a stale slot still points at: every frame equals a fresh renderer's frame of the same scene."""
    sc = scenes.textured_scene(5, 16)
    cell = scenes.min_cell(sc)
    p = v.default_params(200, 112, cell, 255, shadow=True, mode=_abi.MODE_INTERP)

    def fresh():
        r2 = v.VHipRenderer()
        assert r2.Start()
        try:
            return gpu_render(r2, sc, p)[0]
        finally:
            r2.Stop()

    r = v.VHipRenderer()
    assert r.Start()
    try:
        first, _ = gpu_render(r, sc, p)
        assert np.array_equal(first, fresh())
        vols = sc.volumes()
        alb2, nrm2, rm2 = scenes.procedural_textures(77)
        vols[0].Material.AlbedoTexture = alb2          # swapped: the old albedo image stays bound to volume 1
        swapped, _ = gpu_render(r, sc, p)
        assert not np.array_equal(swapped, first) and np.array_equal(swapped, fresh())
        vols[1].Material.AlbedoTexture = None          # now no volume names the old albedo image: its id is freed ...
        vols[2].Material.RMTexture = rm2               # ... and handed to this new image in the same sync
        vols[2].Material.TextureScale = (29.0, 31.0)
        again, _ = gpu_render(r, sc, p)
        assert not np.array_equal(again, swapped) and np.array_equal(again, fresh())
        vols[0].Material.Roughness = 0.45              # a scalar edited in place reaches the device as well
        rough, _ = gpu_render(r, sc, p)
        assert not np.array_equal(rough, again) and np.array_equal(rough, fresh())
        assert len(set(r._tex_ids.values())) == len(r._tex_ids) <= 4
    finally:
        r.Stop()


def test_scene_swap_with_more_textures_than_fit_together(oracle_lib):
    """two scenes of 33 material textures each (11 volumes x albedo / normal / RM) given to ONE renderer in turn: the
    old scene's images leave the device before the new ones arrive (66 > VRT_MAX_TEXTURES = 64 would not fit together), no slot
    ever names a freed id, and every frame equals a fresh renderer's."""
    def scene(seed):
        rng = np.random.default_rng(seed)
        objs = []
        for k in range(11):
            m = v.VMaterial(tuple(rng.uniform(0.3, 1.0, 3)) + (1.0,), 0.7, 0.1)
            tex = []
            for _ in range(3):
                t = rng.integers(40, 255, size=(2, 3, 4), dtype=np.uint8)
                t[..., 2] = 230
                t[..., 3] = 255
                tex.append(t)
            m.AlbedoTexture, m.NormalTexture, m.RMTexture, m.TextureScale = tex[0], tex[1], tex[2], (17.0, 13.0)
            vol = v.sphere_volume(3, 100.0, 60.0, m)
            objs.append(v.VVoxelObject(Position=(0.0, (k - 5) * 70.0, (k % 3 - 1) * 80.0), Scale=(0.3, 0.3, 0.3), Volume=vol))
        return v.VScene(Camera=v.look_minus_x_camera(500.0), DirectionalLight=v.demo_light(), Objects=objs, EnvironmentMap=v.procedural_skybox(8))

    a, b = scene(1), scene(2)
    p = v.default_params(240, 136, scenes.min_cell(a), 255, shadow=True, mode=_abi.MODE_INTERP)

    def fresh(sc):
        r2 = v.VHipRenderer()
        assert r2.Start()
        try:
            return gpu_render(r2, sc, p)[0]
        finally:
            r2.Stop()

    fa, fb = fresh(a), fresh(b)
    assert not np.array_equal(fa, fb)
    r = v.VHipRenderer()
    assert r.Start()
    try:
        for sc, want in ((a, fa), (b, fb), (a, fa), (b, fb)):
            got, _ = gpu_render(r, sc, p)
            assert np.array_equal(got, want)
            assert len(r._tex_ids) == 33 and max(r._tex_ids.values()) < _abi.VRT_MAX_TEXTURES
    finally:
        r.Stop()


def test_texture_table_through_the_abi(oracle_lib):
    """vrt_texture_upload / vrt_texture_free / vrt_volume_set_textures: argument checks, replacing an image in place,
    freeing a bound texture (reads as unbound afterwards)."""
    import ctypes as C

    lib = _abi.load()
    sc = scenes.config2_sphere(5, 16)
    vol = sc.volumes()[0]
    cell = scenes.min_cell(sc)
    r = v.VHipRenderer()
    assert r.Start()
    try:
        p = v.default_params(160, 90, cell, 128, shadow=True, mode=_abi.MODE_INTERP)
        base, _ = gpu_render(r, sc, p)
        ctx = r._ctx

        def raw_render():
            """vrt_render without the host mirror's SyncWithScene (which would bind the slot to vol.Material's images again)."""
            out = np.empty((p.height, p.width, 4), np.float32)
            _abi.check(lib.vrt_render(ctx, C.byref(p), out.ctypes.data_as(C.c_void_p)), "vrt_render")
            return out

        red = np.full((2, 2, 4), 64, np.uint8)  # a dark grey image: albedo drops to a quarter of the tint
        red[..., 3] = 255
        assert lib.vrt_texture_upload(ctx, 64, 2, 2, red.ctypes.data_as(C.c_void_p)) == _abi.VRT_ERR_INVALID
        assert lib.vrt_texture_upload(ctx, 3, 0, 2, red.ctypes.data_as(C.c_void_p)) == _abi.VRT_ERR_INVALID
        assert lib.vrt_texture_free(ctx, 3) == _abi.VRT_ERR_SLOT
        assert lib.vrt_volume_set_textures(ctx, 0, 3, -1, -1, 100.0, 100.0) == _abi.VRT_ERR_SLOT      # texture 3 not uploaded
        assert lib.vrt_texture_upload(ctx, 3, 2, 2, red.ctypes.data_as(C.c_void_p)) == 0
        assert lib.vrt_volume_set_textures(ctx, 0, 3, -1, -1, 0.0, 100.0) == _abi.VRT_ERR_INVALID
        assert lib.vrt_volume_set_textures(ctx, 5, 3, -1, -1, 100.0, 100.0) == _abi.VRT_ERR_SLOT     # empty volume slot
        assert lib.vrt_volume_set_textures(ctx, 0, 3, -1, -1, 100.0, 100.0) == 0
        img_red = raw_render()
        vol.Material.AlbedoTexture = red
        ref, _ = OracleScene(sc).render(p, threads=8)
        vol.Material.AlbedoTexture = None
        assert np.abs(img_red - ref).max() <= TOL and np.abs(img_red - base).max() > 0.05
        white = np.full((2, 2, 4), 255, np.uint8)
        assert lib.vrt_texture_upload(ctx, 3, 2, 2, white.ctypes.data_as(C.c_void_p)) == 0         # replace in place
        img_white = raw_render()
        assert np.abs(img_white - img_red).max() > 0.05 and np.abs(img_white - base).max() <= 2e-6   # white = identity
        assert lib.vrt_texture_free(ctx, 3) == 0                                                     # bound texture freed -> unbound
        assert np.array_equal(raw_render(), base)
    finally:
        r.Stop()


@pytest.mark.parametrize("mesh,resolution", [("cube", 5), ("torus", 6), ("torus", 8)])
def test_device_voxelizer_matches_the_cpu_converter(mesh, resolution):
    """vrt_voxelize_mesh (one workgroup per triangle, atomicMin on ordered keys) against the C++ CPU converter
    (VVolumeConverter, csrc/host/VolumeConverter.cpp): every density and material of the volume, bit for bit —
    the reference's config 1 (unit cube -> 32^3) and the config 3 mesh at 64^3 and 256^3."""
    from volumetricraytracer_amd import voxelizer as vx

    pos, _, idx = vx.cube_mesh() if mesh == "cube" else vx.torus_mesh(0.55, 0.22, 128, 64)
    p, be = vx.importer_space(pos)
    cpu = vx.convert_mesh(p, idx, be, f"{mesh}_{resolution}")
    r = v.VHipRenderer()
    assert r.Start()
    try:
        skipped = r.voxelize_mesh(2, p, idx, resolution, cpu.VolumeExtends)
        gpu = r.download_volume(2, resolution, cpu.VolumeExtends)
        assert skipped == 0
        assert np.array_equal(gpu.density, cpu.density)
        assert np.array_equal(gpu.material_id, cpu.material_id)
        assert (gpu.density <= 0).sum() > 100 and gpu.density.max() == np.float32(cpu.VolumeExtends * 2)
        if mesh == "cube":
            # the whole grid, far voxels and background included, against the float64 reference (tests/voxelize_ref.py)
            import voxelize_ref as V

            tri, none_skipped = V.usable(p, idx)
            ref = V.reference(tri, resolution, cpu.VolumeExtends)
            assert none_skipped == 0 and ref.ambiguous == 0 and V.well_conditioned(tri, cpu.GetCellSize()).all()
            assert (np.abs(gpu.density - ref.density) <= V.tol(gpu.N, ref.density)).all(), V.scaled_error(gpu.N, gpu.density, ref.density)
            assert (~ref.covered).sum() > 1000 and (gpu.density[~ref.covered] == np.float32(cpu.VolumeExtends * 2)).all()
            sure = np.abs(ref.density) > V.tol(gpu.N, ref.density)
            assert (~sure).sum() <= V.LEFT_OUT_SHARE * sure.size and np.array_equal(gpu.material_id[sure], ref.material[sure])
        # the slot renders like an uploaded copy of the CPU volume (metric set by the voxelizer itself)
        if resolution <= 6:
            cpu.Material = v.VMaterial((0.8, 0.6, 0.2, 1.0), 0.8, 0.0)
            sc = v.VScene(Camera=v.look_minus_x_camera(cpu.VolumeExtends * 3.0), DirectionalLight=v.demo_light(), Objects=[v.VVoxelObject(Volume=cpu)])
            prm = v.default_params(160, 90, cpu.GetCellSize(), 255, shadow=True)
            want, _ = gpu_render(r, sc, prm)                      # slot 0: uploaded CPU volume
            abi_scene = sc.to_abi()
            abi_scene.instances[0].volume_slot = 2                # same scene, instance points at the voxelized slot
            mat = cpu.Material.to_abi()
            _abi.check(r._lib.vrt_volume_set_material(r._ctx, 2, C.byref(mat)), "vrt_volume_set_material")
            _abi.check(r._lib.vrt_scene_set(r._ctx, C.byref(abi_scene)), "vrt_scene_set")
            got = np.empty_like(want)
            _abi.check(r._lib.vrt_render(r._ctx, C.byref(prm), got.ctypes.data_as(C.c_void_p)), "vrt_render")
            assert np.array_equal(got, want)
        # degenerate and out-of-range triangles are skipped and counted, like the CPU converter does
        bad = np.concatenate([idx.reshape(-1), np.array([0, 0, 1, 0, 1, len(p) + 5], np.uint32)])
        assert r.voxelize_mesh(3, p, bad, min(resolution, 5), cpu.VolumeExtends) == 2
    finally:
        r.Stop()


def test_voxelizer_cli_on_the_device_writes_the_same_file(tmp_path):
    """`voxelizer --gpu scene.gltf` (glTF import and .vox export on the host, the per-triangle loop through
    vrt_voxelize_mesh + vrt_volume_download) against the plain CPU run of the same tool: identical bytes."""
    import subprocess

    from volumetricraytracer_amd import voxelizer as vx

    pos, nrm, idx = vx.torus_mesh(0.55, 0.22, 64, 32)
    cpos, cnrm, cidx = vx.cube_mesh(0.5)
    gltf = str(tmp_path / "scene.gltf")
    nodes = [{"name": "Torus", "mesh": 0, "translation": [0.0, 0.0, 1.0]}, {"name": "Cube", "mesh": 1, "scale": [1.0, 2.0, 0.5]},
             {"name": "Light_Sun", "rotation": [0.0, 0.0, 0.0, 1.0], "extras": {"strength": 6.0}}]
    vx.write_gltf(gltf, [("torus_6", pos, nrm, idx, None), ("cube_5", cpos, cnrm, cidx, None)], nodes)
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "voxelizer")
    cpu_out, gpu_out = str(tmp_path / "cpu.vox"), str(tmp_path / "gpu.vox")
    r1 = subprocess.run([exe, "--out", cpu_out, gltf], capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([exe, "--gpu", "--out", gpu_out, gltf], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0 and "host voxelizer" in r1.stdout, r1.stderr
    assert r2.returncode == 0 and "device voxelizer" in r2.stdout and "failed" not in r2.stdout, r2.stdout + r2.stderr
    a, b = open(cpu_out, "rb").read(), open(gpu_out, "rb").read()
    assert len(a) > 2_000_000 and a == b


@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
@pytest.mark.parametrize("path", [_abi.PATH_BRICK, _abi.PATH_DENSE, _abi.PATH_BRICK_LDS, _abi.PATH_CELLS])
def test_shell_volume_paths_and_formats_parity(renderer, oracle_lib, path, fmt):
    """Voxelizer shell volumes march with the two-level empty-space table (brick bytes + sub-block nibbles) and never
    sample where it shows no active cell.  Every data path (int16 bricks when the volume is in the reference's texel
    format) on the single-instance scene, the instanced scene (BVH) and the full closest hit: pixels <= 1e-4, every
    counter exact where the traversal order is the oracle's, and all paths bit-identical to each other."""
    sc = scenes.config3_voxelized(6, 16, device_format=fmt)
    p = v.default_params(320, 180, scenes.min_cell(sc), 255, shadow=True, path=path)
    img, t = assert_parity(renderer, sc, p)
    assert 0 < t["shadow_rays"] < t["hits"]
    q = v.default_params(320, 180, scenes.min_cell(sc), 255, shadow=True, path=_abi.PATH_DENSE)
    other, _ = gpu_render(renderer, sc, q)
    assert np.array_equal(img, other)
    shell_instances = scenes.config5_instances(5, 16)
    vol = scenes.voxelized_torus(5).set_device_format(fmt)
    for o in shell_instances.Objects:
        o.Volume = vol
    p = v.default_params(240, 136, vol.GetCellSize(), 255, shadow=True, path=path)
    assert_parity(renderer, shell_instances, p, check_stats=False)
    full = scenes.full_closest_hit_scene()
    for vv in full.volumes():
        vv.set_device_format(fmt)
    p = v.default_params(240, 136, scenes.min_cell(full), 255, shadow=True, path=path)
    p.max_bounces = 2
    assert_parity(renderer, full, p, check_stats=False)


@pytest.mark.parametrize("k_relax", [0.6, 1.0, 1.3, 1.7, 2.0])
def test_over_relaxation_factors_parity(renderer, oracle_lib, k_relax):
    """vrt_params.k_relax: below 1 every step is scaled down, 1 is plain sphere tracing, above 1 steps are stretched and
    checked by the overlap of successive empty spheres (the march goes back where they do not overlap).  Every factor, on the
    Voxelizer shell (tables, clamp), a metric SDF (no clamp, no tables), an instanced scene through the BVH (the stretched
    steps depend on the interval's end: the result must not depend on the visiting order) and a one-cell-thick shell (the
    worst case for a stretched step): pixels <= 1e-4 and counters exact against the oracle on the per-lane and the LDS paths;
    for the thin shell also the same hit mask as plain sphere tracing."""
    shell = scenes.config3_voxelized(6, 16)
    for path in (_abi.PATH_BRICK, _abi.PATH_BRICK_LDS, _abi.PATH_DENSE):
        p = v.default_params(256, 144, scenes.min_cell(shell), 255, shadow=True, path=path, k_relax=k_relax)
        assert_parity(renderer, shell, p)
    sdf = scenes.config3_torus(6, 16)
    assert_parity(renderer, sdf, v.default_params(256, 144, scenes.min_cell(sdf), 255, shadow=True, k_relax=k_relax))
    inst = scenes.config5_instances(5, 16)
    assert_parity(renderer, inst, v.default_params(240, 136, scenes.min_cell(inst), 255, shadow=True, k_relax=k_relax), check_stats=False)
    vol = v.VVoxelVolume(6, 100.0)
    half = 0.5 * float(vol.GetCellSize())
    vol.fill(lambda X, Y, Z: np.abs(np.sqrt(X * X + Y * Y + Z * Z) - 60.0) - half)
    thin = v.VScene(Camera=sdf.Camera, DirectionalLight=sdf.DirectionalLight, Objects=[v.VVoxelObject(Volume=vol)])

    def unlit(k):
        q = v.default_params(256, 144, vol.GetCellSize(), 255, shadow=False, k_relax=k)
        q.mode = _abi.MODE_INTERP_NOTEX_UNLIT  # a hit pixel is the tint, a miss is black (no sky box)
        return q

    img, t = assert_parity(renderer, thin, unlit(k_relax))
    plain, t1 = gpu_render(renderer, thin, unlit(1.0))
    hit, hit1 = img[..., :3].sum(axis=2) > 0, plain[..., :3].sum(axis=2) > 0
    # silhouette pixels may differ, nothing inside the disc may: every differing pixel lies within one pixel of the plain
    # trace's silhouette (a hole torn by a stretched step would sit inside the eroded disc)
    assert hit1.mean() > 0.05 and (hit != hit1).mean() < 0.002
    assert not (hit & ~_dilate(hit1)).any() and not (_erode(hit1) & ~hit).any()
    assert abs(t["hits"] - t1["hits"]) <= 0.002 * img.shape[0] * img.shape[1]


def _dilate(mask):
    """3x3 dilation of a boolean image."""
    m = np.pad(mask, 1)
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= m[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


def _erode(mask):
    return ~_dilate(~mask)


@pytest.mark.parametrize("k_relax", [1.0, 1.7])
@pytest.mark.parametrize("fmt", ["f32", "texel16"])
def test_hit_mask_is_the_reference_surface_on_the_benched_volume(renderer, oracle_lib, fmt, k_relax):
    """VERDICT r2 item 2, GPU side: the march over the benched 256^3 Voxelizer shell (step clamp, two-level leap table,
    over-relaxation, overshoot repair) against the REFERENCE's own hit definition.  vrt_render's hit mask at 320x180 (unlit
    mode, no sky box: a hit pixel is the tint, a miss is black) versus the mask vrto_ref_hit_t — the reference's DDA +
    per-cell cubic (SH/Include/Voxel.hlsli:497-538, 552-605, 691-781), double precision, on the very field the march samples —
    gives per pixel: every difference lies within one pixel of the reference silhouette (rays that graze the surface inside
    their own footprint), and less than 1 % of the pixels differ at all."""
    import copy

    W, H = 320, 180
    base = scenes.bench_config3() if fmt == "f32" else scenes.config3_voxelized(8, 16, device_format=_abi.FORMAT_TEXEL16)
    vol = base.volumes()[0]
    sc = v.VScene(Camera=base.Camera, DirectionalLight=base.DirectionalLight, Objects=[v.VVoxelObject(Volume=vol)])
    p = v.default_params(W, H, vol.GetCellSize(), 255, shadow=False, k_relax=k_relax)
    p.mode = _abi.MODE_INTERP_NOTEX_UNLIT
    img, t = gpu_render(renderer, sc, p)
    mask = img[..., :3].sum(axis=2) > 0
    o = OracleScene(sc)
    org, dr = o.camera_rays(W, H, [(x, y) for y in range(H) for x in range(W)])
    if fmt == "texel16":
        vq = copy.copy(vol)
        vq.density, vq.device_format = o.tables(0)[2].copy(), _abi.FORMAT_F32  # the integer field +-q: same zero set
        oref = OracleScene(v.VScene(Camera=sc.Camera, Objects=[v.VVoxelObject(Volume=vq)]))
    else:
        oref = o
    rh, _ = oref.ref_hit_batch(0, org, dr, threads=8)
    ref = rh.reshape(H, W)
    assert 0.1 < ref.mean() < 0.6 and t["exhausted_rays"] == 0
    assert not (mask & ~_dilate(ref)).any(), "a hit far outside the reference's silhouette"
    assert not (_erode(ref) & ~mask).any(), "a hole inside the reference's silhouette"
    assert (mask != ref).mean() < 0.01


# ---- pixel-level pin to the reference's own intersection -----------------------------------------------
# tests/golden/ref_*.npz: frames as the reference's intersection shaders would produce them (exact per-cell cubic root, normal at
# the root; vrto_ref_render, tests/golden/make_ref_golden.py) in the 8-bit colours of its render target.  The fixtures do not
# depend on the sphere-trace's contract.  Bounds: fraction of the interior of the reference's surfaces whose 8-bit colour differs
# by more than 1 / 2 steps (tests/ref_pixels.py); measured values in DESIGN.md §5.
REF_PIXEL_BOUNDS = {
    # (ref_boundarybox16_320x180, a surface within a cell of its volume's box, is test_hip_frame_against_the_literal_reference_frame's: the
    # default boundary rule differs from the reference's there by design)
    "ref_c3vox256_texel16_320x180": (0.002, 0.002),
    "ref_c3vox256_f32_320x180": (0.002, 0.002),
    "ref_c3vox256_texel16_1080p_rows492": (0.001, 0.001),
    "ref_c3vox256_texel16_2160p_rows1040": (0.001, 0.001),   # config 4's frame size (measured 0.00014; rounds 1-3: 0.094)
    "ref_c5inst128_1080p_rows300": (0.0005, 0.0005),          # config 5 at its real size (measured 0.00005 = one pixel; rounds 1-3: 0.024)
    "ref_c2sphere64_320x180": (0.0, 0.0),
    "ref_c5inst32_320x180": (0.0, 0.0),
    # mirror bounces: the reflection of another object's silhouette lies INSIDE the mirror's own surface (measured 0.0073 / 0.0044)
    "ref_fullhit64_320x180": (0.015, 0.01),
    # textured mode (tri-planar albedo / normal / RM maps, point-sampled): a texel boundary next to the hit flips a texel (measured
    # 0.0085 / 0.0076; rounds 1-3: 0.48 — a normal map amplifies the normal's error)
    "ref_textured64_320x180": (0.02, 0.02),
}
_ref_pixel_report = []


def _ref_case(name):
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(GOLDEN, "make_ref_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.build_case(m.CASES[name])


@pytest.mark.parametrize("name", sorted(REF_PIXEL_BOUNDS))
def test_hip_frame_is_the_reference_frame(renderer, name):
    """HIP frames (k_relax 1.0 and 1.7; the float target quantised, and the RGBA8 target itself) against the reference-intersection
    fixtures: the interior of every surface within the bounds above, the whole window (silhouettes included) under 1 %."""
    from tests import ref_pixels

    sc, p, row0, rows = _ref_case(name)
    gt1, gt2 = REF_PIXEL_BOUNDS[name]
    for k_relax in (1.7, 1.0):
        q = _abi.vrt_params.from_buffer_copy(p)
        q.k_relax = k_relax
        img, t = gpu_render(renderer, sc, q)
        m = ref_pixels.compare(img[row0:row0 + rows], name)
        _ref_pixel_report.append((name, k_relax, m))
        print("ref-pixels", name, "k_relax", k_relax, m)
        # (no march runs out of its 255 positions with the default over-relaxation; plain sphere tracing at 3840x2160 — footprints of a
        # twentieth of a cell — leaves a few dozen grazing rays of 8.3 M short, counted as misses: §3.5)
        assert m["interior_pixels"] > 1000 and t["exhausted_rays"] <= (0 if k_relax > 1.0 else 100)
        assert m["gt1"] <= gt1 and m["gt2"] <= gt2, (k_relax, m)
        assert m["frame_gt1"] <= 0.01, (k_relax, m)
    # the 8-bit target the reference presents (VRT_FLAG_OUTPUT_RGBA8) holds exactly the quantised float frame
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= _abi.FLAG_OUTPUT_RGBA8
    img8, _ = gpu_render(renderer, sc, q)
    img, _ = gpu_render(renderer, sc, p)
    assert np.array_equal(np.asarray(img8)[..., :3], ref_pixels.quantise(img))


# ---- "what the DXR backend renders" (round 5): the literal restatement's frames, the two reference flags, constant textures -------------------
REF_FLAGS = _abi.FLAG_REFERENCE_VIEW_VECTOR | _abi.FLAG_REFERENCE_BOUNDARY_TEXELS
# HIP frame with both flags against tests/golden/ref_literal_*.npz (vrto_ref_literal_render: the reference's shaders statement by statement,
# fp32, nudges, octree leaves, three secant steps, un-normalised direction): interior "more than one step" fraction.  Same bounds as the
# oracle's sphere-trace in tests/test_reference_pixels.py (GPU = oracle to 7e-7).
LITERAL_PIXEL_BOUNDS = {
    "ref_c3vox256_texel16_320x180": 0.004,
    "ref_c3vox256_texel16_1080p_rows492": 0.007,
    "ref_c3vox256_texel16_2160p_rows1040": 0.007,
    "ref_c5inst128_1080p_rows300": 0.004,
    "ref_c2sphere64_320x180": 0.002,
    "ref_c5inst32_320x180": 0.001,
    "ref_boundarybox16_320x180": 0.003,
    "ref_fullhit64_320x180": 0.015,
    "ref_textured64_320x180": 0.02,
}


@pytest.mark.parametrize("name", sorted(LITERAL_PIXEL_BOUNDS))
def test_hip_frame_against_the_literal_reference_frame(renderer, oracle_lib, name):
    """HIP <-> literal (bounded), HIP <-> idealised (the fixture of test_hip_frame_is_the_reference_frame) and, on the
    same inputs, HIP = oracle <= 1e-4 with the two reference flags set — the three columns of DESIGN.md §5.0."""
    from tests import ref_pixels

    sc, p, row0, rows = _ref_case(name)
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= REF_FLAGS
    img, t = gpu_render(renderer, sc, q)
    m = ref_pixels.compare(img[row0:row0 + rows], name, against="literal")
    mi = ref_pixels.compare(img[row0:row0 + rows], name, against="idealised")
    print("ref-pixels literal", name, m, "| idealised", mi)
    assert m["interior_pixels"] > 1000 and m["gt1"] <= LITERAL_PIXEL_BOUNDS[name], m
    ref, st = OracleScene(sc).render(q, row0, rows, threads=8)
    assert np.abs(img[row0:row0 + rows] - ref).max() <= TOL


@pytest.mark.parametrize("case", ["lean", "lean_texel16", "bvh", "full_one_kernel", "full_passes", "textured", "boundary", "cube"])
def test_reference_flags_parity(renderer, oracle_lib, case):
    """VRT_FLAG_REFERENCE_VIEW_VECTOR (wo = -L d, secondary rays 0.1 L back) and VRT_FLAG_REFERENCE_BOUNDARY_TEXELS in every kernel form:
    GPU = oracle <= 1e-4 with exact counters, and the frames DIFFER from the un-flagged ones (the flags reach the kernels)."""
    bounces, mode, flags = 0, _abi.MODE_INTERP_NOTEX, REF_FLAGS
    if case == "lean":
        sc = scenes.config3_torus(6, 16)
    elif case == "lean_texel16":
        sc = scenes.config3_voxelized(6, 16, device_format=_abi.FORMAT_TEXEL16)
    elif case == "bvh":
        sc = scenes.config5_instances(5, 16)
    elif case in ("full_one_kernel", "full_passes"):
        sc, bounces = scenes.full_closest_hit_scene(5, 16), 2
        flags |= _abi.FLAG_FULL_THREE_PASS if case == "full_passes" else 0
    elif case == "textured":
        sc, bounces, mode = scenes.textured_scene(5, 16), 2, _abi.MODE_INTERP
    elif case == "boundary":
        sc = scenes.boundary_box_scene(4, 16)
    else:
        sc, mode = scenes.config3_torus(5, 16), _abi.MODE_CUBE_NOTEX
    p = v.default_params(192, 108, scenes.min_cell(sc), 255, shadow=True, mode=mode)
    p.max_bounces = bounces
    plain, _ = gpu_render(renderer, sc, p)
    plain = plain.copy()
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= flags
    img, t = assert_parity(renderer, sc, q, check_stats=len(sc.Objects) == 1)
    form = renderer.last_kernel_form()
    if case in ("lean", "lean_texel16", "bvh", "boundary", "cube"):
        assert form & _abi.FORM_LEAN_REF and not form & _abi.FORM_FULL
    else:
        assert form & _abi.FORM_FULL and bool(form & _abi.FORM_PASSES) == (case == "full_passes")
    assert np.abs(img - plain).max() > 1e-5  # (even the Cube modes' shading sees the longer view vector)


@pytest.mark.parametrize("case", ["single_f32", "single_texel16", "bvh", "unlit", "mirror_const_rm", "block"])
def test_constant_textures_stay_on_the_lean_kernel(renderer, oracle_lib, case):
    """the reference binds a 1x1 default texture to every unbound material slot (RDXScene.cpp:241-260); its normal texel
    (127, 127, 255) tilts every normal by 0.3 degrees in Interp, its default mode.  A 1x1 texture is a constant: folded into the lean
    kernel (no fetch, 8 waves per SIMD, no full closest hit) with the very arithmetic of the texture path — GPU = oracle (which samples
    the 1x1 image like any other) <= 1e-4, exact counters, and bit-equal to the full closest hit forced onto the same frame."""
    mode, bounces = _abi.MODE_INTERP, 0
    if case == "single_f32":
        sc = scenes.config3_voxelized(6, 16)
    elif case in ("single_texel16", "block"):
        sc = scenes.config3_voxelized(6, 16, device_format=_abi.FORMAT_TEXEL16)
    elif case == "bvh":
        sc = scenes.config5_instances(5, 16)
    elif case == "unlit":
        sc, mode = scenes.config3_torus(5, 16), _abi.MODE_INTERP_UNLIT
    else:
        # a constant RM texel that turns a rough material (0.8) into a mirror (0.8 * 51/255 = 0.16): the host must see it and launch the full form
        sc, bounces = scenes.config3_torus(5, 16), 2
        sc.volumes()[0].Material.RMTexture = np.array([[[51, 255, 0, 255]]], np.uint8)
    scenes.with_reference_default_textures(sc)
    if case in ("bvh", "unlit"):  # every slot a constant: albedo and RM factors too
        for vol in sc.volumes():
            vol.Material.AlbedoTexture = np.array([[[200, 180, 90, 255]]], np.uint8)
            vol.Material.RMTexture = np.array([[[230, 40, 0, 255]]], np.uint8)
    p = v.default_params(192, 108, scenes.min_cell(sc), 255, shadow=True, mode=mode)
    p.max_bounces = bounces
    p.flags |= REF_FLAGS
    if case == "block":
        import torch

        cams = scenes.orbit_cameras(sc, 4)
        renderer.SetSceneToRender(sc)
        renderer.SyncWithScene()
        out = torch.zeros((4, p.height, p.width, 4), dtype=torch.float32, device="cuda")
        renderer.render_block(p, 4, out.data_ptr(), p.height * p.width * 16, 0, cameras=cams, rows=(0, p.height))
        torch.cuda.synchronize()
        form = renderer.last_kernel_form()
        assert form & _abi.FORM_LEAN_REF and form & _abi.FORM_TEXTURED and not form & (_abi.FORM_FULL | _abi.FORM_PASSES)
        import copy

        for f in (0, 3):
            s2 = copy.copy(sc)
            s2.Camera = v.VCamera(Position=cams[f][0], Rotation=cams[f][1], FOVAngle=cams[f][2])
            ref, _ = OracleScene(s2).render(p, threads=8)
            assert np.abs(out[f].cpu().numpy() - ref).max() <= TOL
        return
    img, t = assert_parity(renderer, sc, p, check_stats=len(sc.Objects) == 1)
    form = renderer.last_kernel_form()
    if case == "mirror_const_rm":
        assert form & _abi.FORM_FULL and form & _abi.FORM_MAY_BOUNCE and t["bounce_rays"] > 0
        return
    assert form & _abi.FORM_LEAN_REF and form & _abi.FORM_TEXTURED and not form & _abi.FORM_FULL, form
    # the texel does something (0.3 degrees of tilt: a third of the surface's pixels move by one 8-bit step) ...
    bare = scenes.config3_voxelized(6, 16) if case == "single_f32" else None
    if bare is not None:
        img0, _ = gpu_render(renderer, bare, p)
        assert 1e-4 < np.abs(img0 - img).max() < 0.1
    # ... and the same frame through the full closest hit (a 2x2 copy of the texel is an image to the host): bit-equal
    for vol in sc.volumes():
        for name in ("AlbedoTexture", "NormalTexture", "RMTexture"):
            t1 = getattr(vol.Material, name)
            if t1 is not None:
                setattr(vol.Material, name, np.ascontiguousarray(np.tile(t1, (2, 2, 1))))
    img2, t2 = gpu_render(renderer, sc, p)
    assert renderer.last_kernel_form() & _abi.FORM_FULL
    assert np.array_equal(img2, img) and {k: t2[k] for k in STAT_KEYS} == {k: t[k] for k in STAT_KEYS}


def test_hip_frame_without_the_hit_polish_is_what_rounds_1_to_3_rendered(renderer):
    """VRT_FLAG_NO_HIT_POLISH: the normal where the cone threshold stopped the ray.  A quarter of the interior differs from the
    reference's colours by more than one 8-bit step — the number this round's polish removes."""
    from tests import ref_pixels

    name = "ref_c3vox256_texel16_320x180"
    sc, p, row0, rows = _ref_case(name)
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= _abi.FLAG_NO_HIT_POLISH
    img, _ = gpu_render(renderer, sc, q)
    m = ref_pixels.compare(img[row0:row0 + rows], name)
    print("ref-pixels (no polish)", name, m)
    assert m["gt1"] >= 0.10
    ref, st = OracleScene(sc).render(q, threads=8)
    assert np.abs(img - ref).max() <= TOL


def test_reference_texel_upload_is_the_texel16_format(renderer, oracle_lib):
    """R6: vrt_volume_upload_texels takes the reference's own RGBA8 volume texture (UpdateVolumeTexture,
    RDXVoxelVolume.cpp:294-327).  Same frame, bit for bit, as the fp32 upload in VRT_FORMAT_TEXEL16 (which quantises on the
    device), also after a round trip through vrt_volume_download; a scene mixing both formats marches the dense grids."""
    sc = scenes.config3_voxelized(6, 16, device_format=_abi.FORMAT_TEXEL16)
    vol = sc.volumes()[0]
    p = v.default_params(256, 144, scenes.min_cell(sc), 255, shadow=True)
    a, ta = assert_parity(renderer, sc, p)
    renderer.SetSceneToRender(sc)
    renderer.SyncWithScene()
    renderer.upload_volume(0, vol, as_texels=True)
    buf = np.empty((p.height, p.width, 4), np.float32)
    _abi.check(renderer._lib.vrt_render(renderer._ctx, C.byref(p), buf.ctypes.data_as(C.c_void_p)), "vrt_render")
    assert np.array_equal(a, buf)
    back = renderer.download_volume(0, vol.Resolution, vol.VolumeExtends)
    want = vol.density.copy()
    q = ((np.abs(want) * np.float32(100.0)).astype(np.int64) & 0x7FFF).astype(np.float32) * np.float32(0.01)
    assert np.array_equal(back.density, np.where(want < 0, -q, q).astype(np.float32))
    assert np.array_equal(back.material_id, vol.material_id)
    # mixed formats in one scene
    mixed = scenes.config5_instances(5, 16, distinct_volumes=True)
    for i, vv in enumerate(mixed.volumes()):
        vv.set_device_format(_abi.FORMAT_TEXEL16 if i % 2 else _abi.FORMAT_F32)
    pm = v.default_params(240, 136, scenes.min_cell(mixed), 255, shadow=True)
    assert_parity(renderer, mixed, pm, check_stats=False)
    pm.mode = _abi.MODE_CUBE_NOTEX
    renderer.SetSceneToRender(mixed)
    renderer.SyncWithScene()
    rc = renderer._lib.vrt_render(renderer._ctx, C.byref(pm), None)
    assert rc == _abi.VRT_ERR_UNSUPPORTED  # the one combination without a kernel, refused loudly


@pytest.mark.parametrize("fmt,path", [(_abi.FORMAT_F32, _abi.PATH_BRICK), (_abi.FORMAT_F32, _abi.PATH_DENSE), (_abi.FORMAT_F32, _abi.PATH_BRICK_LDS),
                                      (_abi.FORMAT_TEXEL16, _abi.PATH_BRICK), (_abi.FORMAT_TEXEL16, _abi.PATH_CELLS)])
def test_bench_volume_parity(renderer, oracle_lib, path, fmt):
    """The volume bench.py marches — BASELINE config 3: the 256^3 Voxelizer shell of the torus mesh, shadow ray on — at
    640x360 on every data path and in both device formats: pixels <= 1e-4 on all pixels, all seven counters exact."""
    sc = scenes.bench_config3()
    for vol in sc.volumes():
        vol.set_device_format(fmt)
    try:
        p = v.default_params(640, 360, scenes.min_cell(sc), 255, shadow=True, path=path)
        img, t = assert_parity(renderer, sc, p)
        assert t["hits"] > 30000 and t["exhausted_rays"] == 0
    finally:
        for vol in sc.volumes():
            vol.set_device_format(_abi.FORMAT_F32)


def test_bench_batch_cameras_parity(renderer, oracle_lib):
    """The frames bench.py actually renders: one step is a batch of views of a camera orbiting the config-3 view
    (workloads.orbit_cameras) issued through vrt_render_block.  The first, a middle and the last camera of the batch at
    1920x1080, each against the oracle on 8 bands of 16 rows, and all three bit-equal to the same view rendered alone."""
    import copy
    import torch

    sc = scenes.bench_config3()
    W, H, B = 1920, 1080, 64
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    cams = scenes.orbit_cameras(sc, B)
    assert np.allclose(cams[B // 2][0], sc.Camera.Position) and np.allclose(cams[B // 2][1], sc.Camera.Rotation)  # the workload's own view
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    pick = [0, 17, B - 1]
    block = torch.empty((len(pick), H, W, 4), dtype=torch.float32, device="cuda:0")
    renderer.render_block(p, len(pick), block.data_ptr(), H * W * 16, 0, cameras=[cams[f] for f in pick])
    torch.cuda.synchronize()
    alone = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    for j, f in enumerate(pick):
        sf = copy.copy(sc)
        sf.Camera = v.VCamera(Position=cams[f][0], Rotation=cams[f][1], FOVAngle=cams[f][2])
        img = block[j].cpu().numpy()
        assert _oracle_bands(sf, p, img) <= TOL, f
        renderer.SetSceneToRender(sf)
        renderer.SyncWithScene()
        renderer.render_rows(p, 0, H, alone.data_ptr(), 0)
        torch.cuda.synchronize()
        assert torch.equal(alone, block[j]), f
    assert not torch.equal(block[0], block[2])


def _oracle_bands(sc, p, img, bands=8, rows=16):
    """Oracle comparison on `bands` bands of `rows` rows spread over the frame (the oracle renders row ranges)."""
    o = OracleScene(sc)
    worst = 0.0
    for k in range(bands):
        y0 = min(int((k + 0.5) * p.height / bands) // 16 * 16, p.height - rows)
        ref, _ = o.render(p, y0, rows, threads=8)
        worst = max(worst, float(np.abs(img[y0:y0 + rows] - ref).max()))
    return worst


@pytest.mark.parametrize("sr", [32, 8])
def test_config4_real_frame_in_eight_strip_launches(renderer, oracle_lib, sr):
    """BASELINE config 4 at its real size: the 3840x2160 frame over the 256^3 bench volume rendered as 8 interleaved-strip
    launches (what 8 ranks do, one after the other on this GPU; 8-row strips are bench.py's layout) into compact tiles,
    un-shuffled like rank 0 does: bit-equal to the single-launch 4K frame; and that frame against the oracle on 8 sampled
    16-row bands."""
    import torch

    from volumetricraytracer_amd.tiles import FrameGather

    sc = scenes.bench_config3()
    W, H, n = 3840, 2160, 8
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    dev = torch.device("cuda", 0)
    whole = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    renderer.render_rows(p, 0, H, whole.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fg = FrameGather(H, W, n, 0, dev, dtype=torch.float32, buffers=1, strip_rows=sr)
    rays = 0
    for g in range(n):
        tile = fg.frames[0][g * fg.rows_per:(g + 1) * fg.rows_per]
        renderer.render_strips(p, sr, g, n, fg.strips_per, tile.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rays += renderer.last_timing()["primary_rays"]
    fg.unshuffle(0)
    torch.cuda.synchronize()
    assert rays == W * H
    assert torch.equal(fg.frame(0), whole)
    if sr == 32:
        img = whole.cpu().numpy()
        assert _oracle_bands(sc, p, img) <= TOL


def test_config5_real_size_bands(renderer, oracle_lib):
    """BASELINE config 5 at its real size: 8 instances of a 128^3 volume + skybox at 1920x1080 through the BVH, against
    the oracle on 8 sampled 16-row bands."""
    sc = scenes.config5_instances(7, 256)
    p = v.default_params(1920, 1080, scenes.min_cell(sc), 255, shadow=True)
    img, t = gpu_render(renderer, sc, p)
    assert t["primary_rays"] == 1920 * 1080 and t["hits"] > 100000 and t["exhausted_rays"] == 0
    assert _oracle_bands(sc, p, img) <= TOL


@pytest.mark.parametrize("resolution", [8, 9])
def test_no_ray_runs_out_of_budget_on_closed_surfaces(renderer, resolution):
    """A march that visits max_steps positions while still inside the volume is treated as a miss — a hole in a closed
    surface (the reference paints it red, Raytracing.hlsl:325-334).  With the default budget — the reference's 255
    (Raytracing.hlsl:229) at its largest resolution 8, doubled at 9 where the cells are half the size (march_budget) — no ray
    of the 1080p frame may run out on the Voxelizer shell of the torus, at 256^3 and at 512^3 (the largest volume)."""
    max_steps = v.march_budget(resolution)
    from volumetricraytracer_amd import voxelizer as vx

    pos, _, idx = vx.torus_mesh(0.55, 0.22, 128, 64)
    pts, _ = vx.importer_space(pos)
    sc = scenes.config3_voxelized(6, 16)  # camera, light and sky of config 3; the volume comes from the device Voxelizer
    small = sc.volumes()[0]
    renderer.SetSceneToRender(sc)
    renderer.SyncWithScene()
    extent = small.VolumeExtends
    renderer.voxelize_mesh(0, pts, idx, resolution, extent)
    cell = 2.0 * extent / (1 << resolution)
    p = v.default_params(1920, 1080, cell, max_steps, shadow=True)
    buf = np.empty((p.height, p.width, 4), np.float32)
    _abi.check(renderer._lib.vrt_render(renderer._ctx, C.byref(p), buf.ctypes.data_as(C.c_void_p)), "vrt_render")
    t = renderer.last_timing()
    assert t["hits"] > 300000
    assert t["exhausted_rays"] == 0, t


@pytest.mark.parametrize("kind", ["nan", "inf", "-inf", "mix"])
def test_non_finite_densities_do_not_break_parity(oracle_lib, kind):
    """Volumes with NaN / +-Inf / 1e30 voxels (a corrupt file, an overflowing generator): no NaN pixel, no hang, and the
    kernel still takes exactly the oracle's decisions — same pixels, same sample and hit counters — in the interpolated
    and in the Cube modes."""
    rng = np.random.default_rng(3)
    sc = scenes.config2_sphere(5, 16)
    vol = sc.volumes()[0]
    vol.density = np.array(vol.density, dtype=np.float32, copy=True)
    vals = {"nan": [np.nan], "inf": [np.inf], "-inf": [-np.inf], "mix": [np.nan, np.inf, -np.inf, 1e30, -1e30]}[kind]
    for j, (a, b, c) in enumerate(rng.integers(0, vol.N, size=(400, 3))):
        vol.density[a, b, c] = vals[j % len(vals)]
    r = v.VHipRenderer()
    assert r.Start()
    try:
        for mode in (_abi.MODE_INTERP_NOTEX, _abi.MODE_CUBE_NOTEX):
            p = v.default_params(160, 90, vol.GetCellSize(), 255, shadow=True, mode=mode)
            img, t = assert_parity(r, sc, p)
            assert t["hits"] > 100
    finally:
        r.Stop()


def test_largest_volume_parity(oracle_lib):
    """Resolution 9 (N = 513, 135 M voxels: 540 MB dense, 1.07 GB of bricks), the largest the 32-bit addressing
    takes (VRT_MAX_RESOLUTION): every path against the oracle; resolution 10 is refused."""
    res = 9
    N = (1 << res) + 1
    g = (np.arange(N, dtype=np.float32) * np.float32(200.0 / (N - 1)) - np.float32(100.0))
    vol = v.VVoxelVolume(res, 100.0)
    X, Z, Y = g[:, None, None], g[None, :, None], g[None, None, :]  # density axes are (x, z, y)
    vol.density = (np.sqrt(X * X + Y * Y + Z * Z) - np.float32(70.0)).astype(np.float32)  # sphere that reaches the far corners' bricks
    vol.Material = v.VMaterial((0.7, 0.8, 0.9, 1.0), 0.8, 0.0)
    sc = v.VScene(Camera=v.look_minus_x_camera(260.0, 30.0), DirectionalLight=v.demo_light(), Objects=[v.VVoxelObject(Volume=vol)],
                  EnvironmentMap=v.procedural_skybox(16))
    r = v.VHipRenderer()
    assert r.Start()
    try:
        for path in (_abi.PATH_BRICK, _abi.PATH_DENSE):
            p = v.default_params(256, 144, vol.GetCellSize(), 255, shadow=True, path=path)
            img, t = assert_parity(r, sc, p)
            assert t["hits"] > 3000
        p = v.default_params(256, 144, vol.GetCellSize(), 255, shadow=True, mode=_abi.MODE_CUBE_NOTEX)
        assert_parity(r, sc, p)
        one = np.zeros(8, np.float32)
        assert r._lib.vrt_volume_upload(r._ctx, 1, 10, 100.0, one.ctypes.data_as(C.c_void_p), None) == _abi.VRT_ERR_INVALID
    finally:
        r.Stop()


def test_cube_mode_edge_cases(renderer, oracle_lib):
    """Camera inside the volume and inside a solid voxel, 1-step budget, ragged frame, resolution 0 and 1."""
    sc = scenes.config2_sphere(5, 16)
    cell = scenes.min_cell(sc)
    for cam in ((20.0, 3.0, 2.0), (60.0, 1.0, -2.0)):  # inside the solid sphere; inside the volume, outside the sphere
        sc.Camera = v.VCamera(Position=cam, Rotation=sc.Camera.Rotation)
        assert_parity(renderer, sc, v.default_params(101, 57, cell, 255, shadow=True, mode=_abi.MODE_CUBE_NOTEX))
    sc = scenes.config2_sphere(5, 16)
    assert_parity(renderer, sc, v.default_params(64, 36, cell, 1, mode=_abi.MODE_CUBE_NOTEX))
    assert_parity(renderer, sc, v.default_params(64, 36, cell, 0, mode=_abi.MODE_CUBE_NOTEX))
    for res in (0, 1):
        vol = v.VVoxelVolume(res, 50.0).fill(lambda X, Y, Z: np.sqrt(X * X + Y * Y + Z * Z) - 40.0)
        s2 = v.VScene(Objects=[v.VVoxelObject(Volume=vol)], Camera=v.look_minus_x_camera(300.0), DirectionalLight=v.demo_light())
        assert_parity(renderer, s2, v.default_params(64, 36, vol.GetCellSize(), 255, shadow=True, mode=_abi.MODE_CUBE_NOTEX))


@pytest.mark.parametrize("name", ["config2_64x36", "config3_96x54", "config5_96x54", "config3vox_96x54", "config3vox_texel16_96x54"])
def test_against_frozen_golden_images(renderer, name):
    from golden.make_golden import CASES, build_case

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    sc, p = build_case(CASES[name])
    img, t = gpu_render(renderer, sc, p)
    assert np.abs(img - g["image"]).max() <= TOL
    if name != "config5_96x54":
        assert [t[k] for k in ("primary_rays", "shadow_rays", "primary_steps", "shadow_steps", "hits")] == [int(x) for x in g["stats"]]


def test_edge_cases(renderer, oracle_lib):
    # ragged frame sizes (not multiples of the 16x16 workgroup tile), 1x1, tall and wide
    sc = scenes.config2_sphere(5, 8)
    cell = scenes.min_cell(sc)
    for (w, h) in [(1, 1), (17, 9), (33, 47), (250, 3), (3, 250)]:
        assert_parity(renderer, sc, v.default_params(w, h, cell, 64))
        assert_parity(renderer, sc, v.default_params(w, h, cell, 64, path=_abi.PATH_BRICK_LDS))
    # camera inside the volume (tEnter < 0), inside the solid, and looking away
    for pos in [(60.0, 0.0, 0.0), (10.0, 5.0, 0.0), (-300.0, 0.0, 0.0)]:
        sc.Camera = v.VCamera(Position=pos, Rotation=sc.Camera.Rotation)
        assert_parity(renderer, sc, v.default_params(96, 54, cell, 64, shadow=True))
        assert_parity(renderer, sc, v.default_params(96, 54, cell, 64, shadow=True, path=_abi.PATH_BRICK_LDS))
    # max_steps = 0 and a 1-step budget: everything misses / only entry hits
    sc = scenes.config2_sphere(5, 8)
    assert_parity(renderer, sc, v.default_params(64, 36, cell, 0))
    assert_parity(renderer, sc, v.default_params(64, 36, cell, 1))
    # smallest grids: resolution 0 (one cell) and 1
    for r in (0, 1, 2):
        vol = v.VVoxelVolume(r, 50.0).fill(lambda X, Y, Z: np.sqrt(X * X + Y * Y + Z * Z) - 30.0)
        s2 = v.VScene(Camera=v.look_minus_x_camera(200.0), DirectionalLight=v.demo_light(), Objects=[v.VVoxelObject(Volume=vol)])
        assert_parity(renderer, s2, v.default_params(64, 36, vol.GetCellSize(), 64, shadow=True))
        assert_parity(renderer, s2, v.default_params(64, 36, vol.GetCellSize(), 64, shadow=True, path=_abi.PATH_BRICK_LDS))
    # empty scene: every ray reads the environment (or black without one)
    s3 = v.VScene(Camera=v.look_minus_x_camera(200.0), EnvironmentMap=v.procedural_skybox(8))
    assert_parity(renderer, s3, v.default_params(64, 36, 1.0, 64))
    s3.EnvironmentMap = None
    img, _ = assert_parity(renderer, s3, v.default_params(64, 36, 1.0, 64))
    assert (img[..., :3] == 0).all() and (img[..., 3] == 1).all()


def test_shell_volume_with_step_clamp(renderer, oracle_lib):
    """Non-metric density (Voxelizer-style shell): density_scale and step_max drive the march."""
    vol = v.VVoxelVolume(6, 100.0)
    thr = vol.GetCellSize() * np.sqrt(3.0)

    def shell(X, Y, Z):  # unsigned distance to a sphere surface, in units of thr, minus 0.5; clamped background
        d = np.abs(np.sqrt(X * X + Y * Y + Z * Z) - 50.0) / thr - 0.5
        return np.where(d < 1.0, d, 200.0)

    vol.fill(shell)
    vol.density_scale = float(thr)
    vol.step_max = float(0.5 * thr)
    sc = v.VScene(Camera=v.look_minus_x_camera(250.0), DirectionalLight=v.demo_light(), Objects=[v.VVoxelObject(Volume=vol)],
                  EnvironmentMap=v.procedural_skybox(8))
    img, t = assert_parity(renderer, sc, v.default_params(320, 180, vol.GetCellSize(), 255, shadow=True))
    assert t["primary_steps"] / t["hits"] > 2 and t["hits"] > 3000  # several clamped steps near the shell per hit; the rest is skipped
    assert_parity(renderer, sc, v.default_params(320, 180, vol.GetCellSize(), 255, shadow=True, path=_abi.PATH_BRICK_LDS))


def test_row_tiles_into_device_memory(renderer, oracle_lib):
    """vrt_render_rows: asynchronous tile render into caller-owned device memory (torch tensor)."""
    import torch

    sc = scenes.config3_torus(6, 16)
    p = v.default_params(200, 120, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.SyncWithScene()
    ref, st = OracleScene(sc).render(p, threads=8)
    full = torch.empty((120, 200, 4), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    steps = 0
    for row0, rows in [(0, 37), (37, 50), (87, 33)]:
        tile = full[row0:row0 + rows]
        renderer.render_rows(p, row0, rows, tile.data_ptr(), stream)
        torch.cuda.synchronize()
        t = renderer.last_timing()
        steps += t["primary_steps"]
        assert t["primary_rays"] == rows * 200 and t["kernel_ms"] > 0
    assert np.abs(full.cpu().numpy() - ref).max() <= TOL
    assert steps == st["primary_steps"]
    hist = renderer.timing_history(3)
    assert len(hist) == 3 and all(h > 0 for h in hist)


def test_interleaved_strips_into_device_memory(renderer, oracle_lib):
    """vrt_render_strips: rank g of 3 renders strips g, g+3, … into a compact tile; the union is the
    oracle frame (ragged last strip; strip slots beyond the frame stay untouched); counters add up."""
    import torch

    from volumetricraytracer_amd.tiles import strip_frame_rows, strip_layout

    W, H, world, sr = 200, 100, 3, 8
    sc = scenes.config3_torus(6, 16)
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.SyncWithScene()
    ref, st = OracleScene(sc).render(p, threads=8)
    total, per = strip_layout(H, world, sr)
    assert (total, per) == (13, 5)
    frame = np.full((H, W, 4), np.nan, np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    rays = steps = 0
    for g in range(world):
        tile = torch.full((per * sr, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
        renderer.render_strips(p, sr, g, world, per, tile.data_ptr(), stream)
        torch.cuda.synchronize()
        t = renderer.last_timing()
        rays += t["primary_rays"]
        steps += t["primary_steps"] + t["shadow_steps"]
        host = tile.cpu().numpy()
        touched = np.zeros(per * sr, bool)
        for local0, frame0, rows in strip_frame_rows(H, world, g, sr):
            frame[frame0:frame0 + rows] = host[local0:local0 + rows]
            touched[local0:local0 + rows] = True
        assert (host[~touched] == -7.0).all()  # rows beyond the frame are skipped
    assert rays == W * H and steps == st["primary_steps"] + st["shadow_steps"]
    assert np.abs(frame - ref).max() <= TOL
    with pytest.raises(_abi.VrtError):
        renderer.render_strips(p, sr, 3, 3, per, tile.data_ptr(), stream)  # first_strip must be < strip_stride
    with pytest.raises(_abi.VrtError):
        renderer.render_strips(p, 0, 0, 3, per, tile.data_ptr(), stream)


def test_rgba8_output_is_the_quantised_float_frame(renderer, oracle_lib):
    """VRT_FLAG_OUTPUT_RGBA8 (the reference's 8-bit UNORM back-buffer precision, DXConstants.cpp:21): the
    same pixels as the float4 path, stored as (uint)(min(c,1)*255+0.5).  Bit-exact against the float
    frame of the same kernel; within 1 LSB of the quantised oracle frame (a 1e-4 float difference can
    straddle a rounding boundary) with almost every byte equal."""
    from test_tiles_gloo import quantize_rgba8

    sc = scenes.config5_instances(5, 16)
    p = v.default_params(320, 180, scenes.min_cell(sc), 255, shadow=True)
    img, _ = gpu_render(renderer, sc, p)
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= _abi.FLAG_OUTPUT_RGBA8
    img8, t8 = gpu_render(renderer, sc, q)
    assert img8.dtype == np.uint8 and img8.shape == (180, 320, 4)
    assert np.array_equal(img8, quantize_rgba8(img))
    assert (img8[..., 3] == 255).all()
    ref, st = OracleScene(sc).render(p, threads=8)
    d = np.abs(img8.astype(np.int16) - quantize_rgba8(ref).astype(np.int16))
    assert d.max() <= 1 and (d != 0).mean() < 1e-3
    assert {k: t8[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}


def test_bench_two_rank_rehearsal(oracle_lib):
    """bench.py's N>1 code path end to end with 2 ranks sharing this box's one GPU (strips, RGBA8 tiles, gather, un-shuffle,
    max-over-ranks timing, counters summed over ranks), started the way the driver starts it — `python bench.py --gpus 2`
    with WORLD_SIZE unset, so bench.py launches its ranks itself.  The tiles travel over gloo via host memory here (RCCL
    needs one GPU per rank); rank 0 checks the gathered frame bit for bit against the frame one GPU renders alone.  A
    rehearsal of the code path, not a measurement."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: val for k, val in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    # VRT_BENCH_NATIVE_PROBE: the rehearsal also walks the N > 1 line's start-up of the C-ABI's own communicator (vrt_comm_init + a
    # 64-byte exchange, in a thread with a deadline).  Two ranks on one GPU is a communicator RCCL cannot build: the run must go on
    # over the other collective and say so — the behaviour a real N-GPU run relies on if RCCL's bootstrap fails or never returns.
    env.update(VRT_BENCH_BACKEND="gloo", VRT_BENCH_VERIFY="1", HSA_ENABLE_IPC_MODE_LEGACY="0", VRT_BENCH_NATIVE_PROBE="1",
               VRT_BENCH_NATIVE_PROBE_DEADLINE_S="45")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", "c2",
           "--full", "--no-cpu-baseline"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["steps"] == 3
    assert out["config"]["width"] == 1280 and out["config"]["height"] == 720  # the SAME frame, split two ways
    assert out["config"]["rays_per_frame"] == 1280 * 720  # config 2 has no shadow rays; every pixel rendered exactly once
    assert out["assembled_frame_equals_single_gpu_frame"] is True
    assert out["value"] > 0 and out["roofline"]["frac"] > 0 and out["latency"]["ms_per_frame"] > 0
    # the default exchange assembles frame g of a block on rank g // 24 (one all-to-all per block of 48); the gather onto rank 0
    # ran as a leg of the same job, and both hold the single-GPU frame; the one-GPU anchor of the curve was measured on rank 0
    assert "all-to-all" in out["config"]["parallelism"] and out["config"]["frames_per_launch"] == 48 and out["config"]["streams"] == 2
    assert "gather" in out["other_exchange"]["exchange"] and out["other_exchange"]["last_frame_equals_single_gpu_frame"] is True
    assert out["scale_anchor"]["value"] > 0 and out["scale_anchor"]["n_gpus"] == 1 and out["speedup_vs_anchor"] > 0
    # the N > 1 line's account of the exchange (round 4): both exchanges with their speed-up over the anchor, the link model's cap
    assert set(out["exchanges"]) == {"rotate", "gather"} and out["exchanges"]["rotate"]["main_line"] and out["exchanges"]["rotate"]["value"] == out["value"]
    assert out["exchanges"]["gather"]["value"] == out["other_exchange"]["value"] and out["link_model"]["gather_to_rank0_cap_Mrays_per_s"] > 0
    assert out["north_star_6x_at_8_gpus"] is None  # (a statement about 8 GPUs only)
    assert "vrt_comm_init unavailable" in out["collective_fallback"] and "torch.distributed" in out["collective"]
    # (round 5) the probe ran on a context of its own, never on the measurement's; what a rank's block time is made of is in the line
    assert out["per_rank"]["march_ms_per_launch"]["max"] >= out["per_rank"]["march_ms_per_launch"]["min"] > 0 and out["per_rank"]["exchange_ms_per_block"] is None
    assert "ONE point" in out["scaling_curve"]
    # a rank count that does not match --gpus is refused, not silently measured
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1"], env=env2, capture_output=True,
                         text=True, timeout=300, cwd=root)
    assert bad.returncode != 0 and "refusing" in bad.stderr


def test_bench_one_gpu_line_has_the_contract_fields(oracle_lib):
    """`python bench.py --full` on one GPU (a short run): ONE JSON line with the driver contract's fields, the `roofline` and
    `cpu_baseline` objects, one stream x 48 frames per launch, launch durations that add up to the timed region (nothing
    overlaps: kernel time x launches per step ~ ms_per_step), and the legs (latency, scale anchor, end to end, config 4)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: val for k, val in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--cpu-seconds", "1"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    o = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in o, k
    assert o["n_gpus"] == 1 and o["steps"] == 3 and o["warmup"] == 1 and o["unit"] == "Mrays/s" and o["vs_baseline"] is None and o["dtype"] == "f32"
    assert o["config"]["width"] == 1920 and o["config"]["height"] == 1080 and o["config"]["streams"] == 1 and o["config"]["frames_per_launch"] == 96
    r = o["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["frames_per_launch"] == 96
    # one stream, ONE launch per 96 frames, 30 launches per step (a step is ~0.11 s): the launches' durations add up to the step's
    assert o["config"]["launches_per_step"] == 30 and o["config"]["frames_per_step"] == 2880 and o["ms_per_step"] > 60.0
    assert 0.85 < r["kernel_ms"] * o["config"]["launches_per_step"] / o["ms_per_step"] <= 1.02
    # the roof the kernel is under: its samples per second against the measured L1 gather ceiling (frac counts cache-served taps)
    # ... measured IN THIS RUN: the ceiling comes from vrt_debug_gather_ceiling on this box, not from a constant
    m = r["measured_in_run"]
    assert m["gather_ceiling_measured_in_run"] is True and 150 < m["gather_ceiling_gsamples_per_s"]["l1"] < 500
    assert m["gather_ceiling_gsamples_per_s"]["l1_coherent_lanes"] > 1.5 * m["gather_ceiling_gsamples_per_s"]["l1"]
    assert m["gather_ceiling_gsamples_per_s"]["mall_hbm"] < m["gather_ceiling_gsamples_per_s"]["l1"]
    assert 0.3 < m["limiter_frac"] < 1.3 and abs(m["limiter_frac"] - m["gevaluations_per_s"] / m["limiter_ceiling_gsamples_per_s"]) < 1e-3
    assert r["limiter_frac"] == m["limiter_frac"] and "yardstick" in m["limiter_note"]
    assert m["trilinear_evaluations_per_launch"] > r["samples_per_launch"]  # + 6 per hit (the normal)
    # ... and what is REPLAYED from the committed PMC passes sits under its own key, tagged, or is absent (another kernel source)
    for k in ("td_busy_frac", "hbm_measured_frac", "valu_issue_frac", "occupancy_mean_waves_per_cu"):
        assert k not in r
    if "replayed_from_profiles" in r:
        assert r["replayed_from_profiles"]["tag"] and "td_busy_frac" in r["replayed_from_profiles"] and "lines_per_vmem_instr" in r["replayed_from_profiles"]
    # value = rays of the batch x steps / time
    assert abs(o["value"] - o["config"]["rays_per_step"] / (o["ms_per_step"] * 1e-3) / 1e6) / o["value"] < 0.01
    c = o["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["chain_positions_max"] > 50
    assert o["latency"]["ms_per_frame"] > o["ms_per_frame"] and o["scale_anchor"]["value"] > 0 and o["end_to_end"]["value"] > 0
    d = o["dynamic_scene"]
    assert d["per_frame_scenes"]["launches_per_batch"] == 1 and d["per_frame_over_static"] > 0.85  # per-frame scene state: ONE launch, close to the standing scene
    fc = o["full_coverage"]
    assert fc["waves_marching"] > 0.85 * fc["waves"] and fc["samples_per_ray"] > o["config"]["samples_per_ray"] and fc["value"] > 0
    assert o["config4"]["value"] > 0 and o["config4"]["scale_anchor"]["value"] > 0
    # the C++ adaptor's defaults (Interp, texel16, the reference's 1x1 default normal texel, BGRA8, reference flags): the LEAN kernel's REF
    # instantiation, within 15 % of the lean kernel in the same formats (block) — round 4 ran this state as a full closest hit at less than half
    dd = o["drop_in_defaults"]
    assert dd["block"]["kernel_form"] == {"full_closest_hit": False, "passes": False, "lean_ref_instantiation": True, "textured": True}
    assert dd["round4_form"]["block"]["kernel_form"]["full_closest_hit"] and dd["round4_form"]["block"]["kernel_form"]["passes"]
    assert dd["block_over_lean"] > 0.85 and dd["block_over_round4_form"] > 1.15 and dd["lone_frame_over_lean"] > 0.8
    assert 0 < o["config"]["marching"]["primary_rays_in_marching_waves"] < o["config"]["marching"]["primary_rays"] == 1920 * 1080


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """`python bench.py --steps N --warmup W` without --full: the contract's line and nothing measured besides it (no CPU baseline,
    no gather ceilings, no legs), a step of the same 30 launches whatever --steps is, and --dump-outputs: what the timed region's
    last launch rendered, within 64 MB, the same from run to run."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: val for k, val in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines, dumps = [], []
    for steps, warmup in ((3, 1), (1, 1)):
        d = tmp_path / f"out{steps}"
        res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                              "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert res.returncode == 0, res.stderr[-2000:]
        js = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1
        lines.append(json.loads(js[0]))
        dumps.append({f.name[:-4]: np.load(f) for f in sorted(d.iterdir())})
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64_000_000
    for o, steps in zip(lines, (3, 1)):
        assert o["steps"] == steps and o["unit"] == "Mrays/s" and o["higher_is_better"] is True and o["dtype"] == "f32"
        assert o["config"]["launches_per_step"] == 30 and o["ms_per_step"] > 60.0
        assert abs(o["value"] - o["config"]["rays_per_step"] / (o["ms_per_step"] * 1e-3) / 1e6) / o["value"] < 0.01
        for k in ("cpu_baseline", "latency", "scale_anchor", "end_to_end", "config4", "reference_texel_format", "full_closest_hit",
                  "no_cull_rect", "dynamic_scene", "full_coverage", "drop_in_defaults"):
            assert o[k] is None, k
        assert o["config"]["marching"] is None and o["roofline"]["measured_in_run"]["gather_ceiling_measured_in_run"] is False
        assert o["roofline"]["frac"] > 0
    # one step is one step: a 1-step run times the same 30 launches as a 3-step run
    assert 0.7 < lines[1]["ms_per_step"] / lines[0]["ms_per_step"] < 1.4
    a, b = dumps
    assert set(a) == {"last_frame", "frames_sample", "frames_sample_index", "last_frame_counters"} == set(b)
    assert a["last_frame"].shape == (1080, 1920, 4) and a["last_frame"].dtype == np.float32
    assert a["frames_sample"].dtype == np.float32 and a["last_frame_counters"].dtype == np.float64
    for k in a:
        assert np.array_equal(a[k], b[k]), k  # same arguments, same inputs, same outputs
    c = dict(zip(("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits", "exhausted_rays"), a["last_frame_counters"]))
    assert c["primary_rays"] == 1920 * 1080 and c["hits"] > 0 and c["shadow_rays"] > 0
    # the sample is drawn from the launch's frames: its pixels of the last camera are the last frame's
    idx = a["frames_sample_index"].astype(np.int64)
    last_cam = idx[:, 0].max()
    mine = idx[:, 0] == last_cam
    assert mine.sum() > 1000 and len(np.unique(idx[:, 0])) == 96
    assert np.array_equal(a["frames_sample"][mine], a["last_frame"][idx[mine, 1], idx[mine, 2]])


def test_native_tile_gather_with_one_rank(oracle_lib):
    """vrt_comm_unique_id / vrt_comm_init / vrt_gather_tiles — RCCL's ncclGather behind the C-ABI, resolved from librccl at
    run time — with the one rank this box has: the gather enqueued on the march stream right behind vrt_render_strips must
    deliver the tile bytes into the frame buffer (world 1: rank-major = the tile itself), without a host synchronisation
    in between.  (With N > 1 the same call sequence runs in bench.py --gather native / native_gather_check.)"""
    import torch

    sc = scenes.config2_sphere(5, 16)
    p = v.default_params(160, 96, scenes.min_cell(sc), 128)
    p.flags |= _abi.FLAG_OUTPUT_RGBA8
    r = v.VHipRenderer()
    assert r.Start()
    try:
        r.SetSceneToRender(sc)
        r.SyncWithScene()
        uid = v.VHipRenderer.comm_unique_id()
        assert len(uid) == _abi.VRT_COMM_ID_BYTES and any(uid)
        r.comm_init(1, 0, uid)
        with pytest.raises(_abi.VrtError):
            r.comm_init(1, 0, uid)  # one communicator per context
        stream = torch.cuda.Stream()
        tile = torch.zeros((96, 160, 4), dtype=torch.uint8, device="cuda:0")
        frame = torch.zeros_like(tile)
        with torch.cuda.stream(stream):
            r.render_strips(p, 32, 0, 1, 3, tile.data_ptr(), stream.cuda_stream)
            r.gather_tiles(tile.data_ptr(), frame.data_ptr(), tile.numel(), 0, stream.cuda_stream)
        torch.cuda.synchronize()
        assert int(frame.sum()) > 0 and torch.equal(frame, tile)
        whole = np.empty((96, 160, 4), np.uint8)
        _abi.check(r._lib.vrt_render(r._ctx, C.byref(p), whole.ctypes.data_as(C.c_void_p)), "vrt_render")
        assert np.array_equal(frame.cpu().numpy(), whole)
        # vrt_exchange_tiles (one group of ncclSend / ncclRecv: frames assembled on rotating ranks) with the one rank: the
        # rank's only chunk comes back to itself, behind a block launch on the same stream
        block = torch.zeros((3, 96, 160, 4), dtype=torch.uint8, device="cuda:0")
        recv = torch.zeros_like(block)
        with torch.cuda.stream(stream):
            r.render_block(p, 3, block.data_ptr(), 96 * 160 * 4, stream.cuda_stream, strips=(32, 0, 1, 3))
            r.exchange_tiles(block.data_ptr(), recv.data_ptr(), block.numel(), stream.cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(recv, block) and torch.equal(recv[2], frame)
        # vrt_comm_expect_sizes (round 5): once the ranks have agreed on the byte counts, any other count is an error code BEFORE RCCL is
        # entered (a size mismatch between ranks would otherwise wait for ever)
        r.comm_expect_sizes(tile.numel(), block.numel())
        with torch.cuda.stream(stream):
            r.gather_tiles(tile.data_ptr(), frame.data_ptr(), tile.numel(), 0, stream.cuda_stream)
            r.exchange_tiles(block.data_ptr(), recv.data_ptr(), block.numel(), stream.cuda_stream)
            with pytest.raises(RuntimeError, match="vrt_gather_tiles"):
                r.gather_tiles(tile.data_ptr(), frame.data_ptr(), tile.numel() // 2, 0, stream.cuda_stream)
            with pytest.raises(RuntimeError, match="vrt_exchange_tiles"):
                r.exchange_tiles(block.data_ptr(), recv.data_ptr(), block.numel() - 4, stream.cuda_stream)
        torch.cuda.synchronize()
        r.comm_expect_sizes(0, block.numel())  # the gather is declared unused: refused; the exchange still runs
        with pytest.raises(RuntimeError, match="vrt_gather_tiles"):
            r.gather_tiles(tile.data_ptr(), frame.data_ptr(), tile.numel(), 0, stream.cuda_stream)
        r.exchange_tiles(block.data_ptr(), recv.data_ptr(), block.numel(), stream.cuda_stream)
        torch.cuda.synchronize()
    finally:
        r.Stop()


def test_frames_in_flight_keep_their_own_scene(oracle_lib):
    """vrt_render_begin / vrt_render_end (the reference's three frames in flight, DXConstants.cpp:23): frame i is begun,
    then the objects, the camera, a light and a material are already changed for frame i+1 (vrt_scene_set,
    vrt_volume_set_material) before frame i is collected.  Every collected frame must be the frame of ITS scene."""
    import copy

    def scene_at(k):
        sc = scenes.config5_instances(5, 16)
        ang = 0.35 * k
        for j, o in enumerate(sc.Objects):
            o.Position = (o.Position[0] + 25.0 * math.sin(ang + j), o.Position[1] - 18.0 * k, o.Position[2] + 9.0 * k)
            o.Rotation = tuple(v.quat_from_axis_angle(v.UP, ang * (j + 1)))
        sc.Camera = v.look_minus_x_camera(900.0 - 40.0 * k, 20.0 * k)
        sc.PointLights = [v.VPointLight(Position=(300.0 - 60.0 * k, 50.0, 200.0), IlluminationStrength=1500.0 + 300.0 * k,
                                        AttenuationLinear=0.01, AttenuationExp=0.0005)]
        sc.volumes()[0].Material = v.VMaterial((0.2 + 0.1 * k, 0.8 - 0.1 * k, 0.5, 1.0), 0.8, 0.1 * k)
        return sc

    import math

    base = scenes.config5_instances(5, 16)
    vol = base.volumes()[0]
    frames = []
    for k in range(7):
        sc = scene_at(k)
        for o in sc.Objects:  # same volume object throughout: it is uploaded once, only the scene around it moves
            o.Volume = vol
        vol.Material = sc_mat = v.VMaterial((0.2 + 0.1 * k, 0.8 - 0.1 * k, 0.5, 1.0), 0.8, 0.1 * k)
        frames.append((sc, copy.copy(sc_mat)))
    r = v.VHipRenderer()
    assert r.Start()
    try:
        K = _abi.VRT_FRAMES_IN_FLIGHT
        r.ResizeRenderOutput(160, 90)
        r.Shadows, r.MaxSteps = True, 255
        pending, got = {}, []
        for k, (sc, mat) in enumerate(frames):
            slot = k % K
            if slot in pending:
                got.append(r.render_end(slot, pending.pop(slot)))
            # the application edits the scene for frame k while frames k-1 and k-2 are still in flight
            vol.Material = mat
            r.SetSceneToRender(sc)
            r.SyncWithScene()  # uploads the volume once (frame 0); afterwards only vrt_scene_set
            mm = mat.to_abi()
            _abi.check(r._lib.vrt_volume_set_material(r._ctx, 0, C.byref(mm)), "vrt_volume_set_material")
            pending[slot] = r.render_begin(slot)
        for k in range(len(frames) - len(pending), len(frames)):
            got.append(r.render_end(k % K, pending.pop(k % K)))
        with pytest.raises(_abi.VrtError):
            r.render_end(0, r.make_params())  # nothing in flight on that slot any more
        # the RGBA8 frame format through the same slots: the quantised version of the float frame of the last scene
        q = r.make_params()
        q.flags |= _abi.FLAG_OUTPUT_RGBA8
        r.render_begin(1, q)
        with pytest.raises(_abi.VrtError):
            r.render_begin(1, q)  # the slot is busy until it is collected
        from test_tiles_gloo import quantize_rgba8
        assert np.array_equal(r.render_end(1, q), quantize_rgba8(got[-1]))
    finally:
        r.Stop()
    assert len(got) == len(frames)
    for k, (sc, mat) in enumerate(frames):
        vol.Material = mat
        p = v.default_params(160, 90, scenes.min_cell(sc), 255, shadow=True)
        p.max_bounces = 2
        ref, _ = OracleScene(sc).render(p, threads=8)
        assert np.abs(got[k] - ref).max() <= TOL, f"frame {k}"
    assert np.abs(got[0] - got[3]).max() > 0.05  # the frames really differ


def test_render_rows_can_be_captured_into_a_graph(renderer, oracle_lib):
    """vrt_render_rows makes no host synchronisation and, after ONE launch of that size on the stream (include/vrt.h), no
    allocation, so a frame can be captured into a HIP graph on that stream and replayed: same pixels as the direct launch; a
    captured launch is not event-timed (0 ms) but its counters are read back.  The captured launch stays replayable after
    later, larger launches on the same and on other streams (its counter buffer is retired, never freed)."""
    import torch

    sc = scenes.config3_torus(6, 16)
    p = v.default_params(200, 120, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.SyncWithScene()
    ref, st = OracleScene(sc).render(p, threads=8)
    direct = torch.zeros((120, 200, 4), dtype=torch.float32, device="cuda:0")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        renderer.render_rows(p, 0, 120, direct.data_ptr(), side.cuda_stream)  # the one warm-up launch the header asks for
    torch.cuda.synchronize()
    out = torch.zeros_like(direct)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        renderer.render_rows(p, 0, 120, out.data_ptr(), side.cuda_stream)
    assert float(out.abs().max()) == 0.0  # capture does not execute
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, direct)
    assert np.abs(out.cpu().numpy() - ref).max() <= TOL
    t = renderer.last_timing()
    assert t["kernel_ms"] == 0.0 and t["primary_steps"] == st["primary_steps"] and t["hits"] == st["hits"]
    # larger launches on the capture stream and on five other streams: the capture stream's counter buffer is outgrown and
    # retired; the graph must still replay into memory that is alive (more streams than there are records, 16, and the
    # take-over of a record: tests/test_launch_streams_gpu.py)
    big = v.default_params(640, 360, scenes.min_cell(sc), 255, shadow=True)
    bigbuf = torch.zeros((360, 640, 4), dtype=torch.float32, device="cuda:0")
    for stream in [side] + [torch.cuda.Stream() for _ in range(5)]:
        with torch.cuda.stream(stream):
            renderer.render_rows(big, 0, 360, bigbuf.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, direct)
    renderer.render_rows(p, 0, 120, direct.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert renderer.last_timing()["kernel_ms"] > 0.0


def test_renderer_releases_textures_of_scenes_it_no_longer_renders(oracle_lib):
    """One renderer, scene after scene, each with three material textures of its own: textures no volume of the current
    scene names leave the device (vrt_texture_free) and their ids are reused — 30 scenes are 90 textures, more than the
    VRT_MAX_TEXTURES slots — and the last scene still renders like the oracle."""
    r = v.VHipRenderer()
    assert r.Start()
    try:
        for i in range(30):
            sc = scenes.textured_scene()
            p = v.default_params(96, 54, scenes.min_cell(sc), 255, shadow=True, mode=_abi.MODE_INTERP)
            img, _ = gpu_render(r, sc, p)
            assert len(r._tex_ids) <= 3
        ref, _ = OracleScene(sc).render(p, threads=8)
        assert np.abs(img - ref).max() <= TOL
    finally:
        r.Stop()


def test_render_block_is_n_frames_in_flight_with_one_call(renderer, oracle_lib):
    """vrt_render_block: a block of frames, each with its own camera, launched on the context's stream pool and ordered
    like ONE asynchronous operation on the caller's stream.  Every frame equals the same frame rendered alone with that
    camera (bit for bit) and the oracle; work the caller enqueued before the block (a fill of the buffer) is seen by no
    frame and work enqueued after it (a copy of the block) sees every frame; only the block's first frame is timed; strips
    mode gives vrt_render_strips' tiles; VRT_FLAG_NO_TIMING switches a single launch's event pair off."""
    import copy
    import torch

    sc = scenes.config3_voxelized(6, 16)
    W, H, n = 200, 120, 11  # more frames than pool streams
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    cam0 = sc.Camera
    cams = []
    for f in range(n):
        a = 0.08 * f
        pos = (cam0.Position[0] * math.cos(a) - cam0.Position[1] * math.sin(a) + 3.0 * f,
               cam0.Position[0] * math.sin(a) + cam0.Position[1] * math.cos(a), cam0.Position[2] - 2.0 * f)
        cams.append((pos, tuple(v.quat_mul(v.quat_from_axis_angle(v.UP, a), cam0.Rotation)), 60.0 - f))
    side = torch.cuda.Stream()
    block = torch.empty((n, H, W, 4), dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(side):
        block.fill_(7.0)  # enqueued BEFORE the block on the caller's stream: no frame may be overwritten by it
        renderer.render_block(p, n, block.data_ptr(), H * W * 16, side.cuda_stream, cameras=cams)
        after = block.clone()  # enqueued AFTER the block: must see every frame
    torch.cuda.synchronize()
    assert torch.equal(after, block) and float(block.max()) <= 1.0
    # ONE launch covered the block's 11 frames (grid.y = frame) and was event-timed
    assert [fr for _, fr in renderer.launch_history(1)] == [n] and renderer.launch_history(1)[0][0] > 0.0
    # ... and with VRT_FLAG_BLOCK_PER_FRAME it is n launches of which only the first is timed: same pixels
    pf = _abi.vrt_params.from_buffer_copy(p)
    pf.flags |= _abi.FLAG_BLOCK_PER_FRAME
    per_frame = torch.empty_like(block)
    renderer.render_block(pf, n, per_frame.data_ptr(), H * W * 16, 0, cameras=cams)
    torch.cuda.synchronize()
    assert torch.equal(per_frame, block)
    hist = renderer.launch_history(n)
    assert hist[0][0] > 0.0 and all(h == 0.0 for h, _ in hist[1:]) and all(fr == 1 for _, fr in hist)
    alone = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    for f in (0, 1, 5, n - 1):
        sf = copy.copy(sc)
        sf.Camera = v.VCamera(Position=cams[f][0], Rotation=cams[f][1], FOVAngle=cams[f][2])
        renderer.SetSceneToRender(sf)
        renderer.SyncWithScene()
        renderer.render_rows(p, 0, H, alone.data_ptr(), 0)
        torch.cuda.synchronize()
        assert torch.equal(alone, block[f]), f
        ref, _ = OracleScene(sf).render(p, threads=8)
        assert np.abs(block[f].cpu().numpy() - ref).max() <= TOL
    assert not torch.equal(block[0], block[n - 1])
    # the scene's own camera is untouched by the block, and a block without cameras repeats the scene's frame
    renderer.SetSceneToRender(sc)
    renderer.SyncWithScene()
    same = torch.empty((3, H, W, 4), dtype=torch.float32, device="cuda:0")
    renderer.render_block(p, 3, same.data_ptr(), H * W * 16, 0)
    renderer.render_rows(p, 0, H, alone.data_ptr(), 0)
    torch.cuda.synchronize()
    assert all(torch.equal(same[f], alone) for f in range(3))
    # strips: rank 1 of 3, RGBA8 tiles, against vrt_render_strips
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= _abi.FLAG_OUTPUT_RGBA8
    per = (((H + 15) // 16) + 2) // 3
    tiles = torch.zeros((4, per * 16, W, 4), dtype=torch.uint8, device="cuda:0")
    one = torch.zeros((per * 16, W, 4), dtype=torch.uint8, device="cuda:0")
    renderer.render_block(q, 4, tiles.data_ptr(), per * 16 * W * 4, 0, strips=(16, 1, 3, per))
    renderer.render_strips(q, 16, 1, 3, per, one.data_ptr(), 0)
    torch.cuda.synchronize()
    assert all(torch.equal(tiles[f], one) for f in range(4)) and int(one.max()) > 0
    # a launch that asks not to be timed
    q.flags |= _abi.FLAG_NO_TIMING
    renderer.render_strips(q, 16, 1, 3, per, one.data_ptr(), 0)
    torch.cuda.synchronize()
    t = renderer.last_timing()
    assert t["kernel_ms"] == 0.0 and t["primary_rays"] > 0
    # ... also through vrt_render (host frame): same pixels, no event pair
    timed_frame, tt = gpu_render(renderer, sc, p)
    pq = _abi.vrt_params.from_buffer_copy(p)
    pq.flags |= _abi.FLAG_NO_TIMING
    untimed_frame, tu = gpu_render(renderer, sc, pq)
    assert np.array_equal(timed_frame, untimed_frame) and tt["kernel_ms"] > 0.0 and tu["kernel_ms"] == 0.0 and tu["hits"] == tt["hits"]
    lib = _abi.load()
    bad = _abi.vrt_block()
    bad.n_frames, bad.rows, bad.frame_stride_bytes = 0, H, H * W * 16
    assert lib.vrt_render_block(renderer._ctx, C.byref(p), C.byref(bad), C.c_void_p(block.data_ptr()), None) == _abi.VRT_ERR_INVALID
    # parameters no launch accepts: a budget beyond the counters' range, a non-positive or NaN relaxation factor, no minimum step
    both_forms = _abi.FLAG_FULL_ONE_KERNEL | _abi.FLAG_FULL_THREE_PASS  # one kernel AND passes: contradictory
    for field, value in (("max_steps", 65536), ("k_relax", 0.0), ("k_relax", float("nan")), ("step_min", 0.0), ("eps_hit", float("nan")),
                         ("flags", both_forms), ("flags", 1 << 20)):
        q2 = _abi.vrt_params.from_buffer_copy(p)
        setattr(q2, field, value)
        assert lib.vrt_render_rows(renderer._ctx, C.byref(q2), 0, H, C.c_void_p(block.data_ptr()), None) == _abi.VRT_ERR_INVALID, field
    bad.n_frames, bad.frame_stride_bytes = 2, H * W * 16 - 16
    assert lib.vrt_render_block(renderer._ctx, C.byref(p), C.byref(bad), C.c_void_p(block.data_ptr()), None) == _abi.VRT_ERR_INVALID


def test_distant_shell_volume_beyond_the_skip_range(renderer, oracle_lib):
    """a Voxelizer shell so far away that a pixel's footprint exceeds half its step clamp (t > t_skip_end): there the
    march samples every position (an inactive cell could produce a hit), and neither the active-box clip nor the host's cull
    rectangle may drop rays by a different rule — rays are clipped only when their whole interval ends before t_skip_end.  Parity
    with the oracle (which states the same rule), on both sides of the boundary and straddling it."""
    base = scenes.config3_voxelized(5, 16)
    vol = base.volumes()[0]
    for dist in (1200.0, 2300.0, 2600.0, 4000.0):  # t_skip_end is about 2500 at 1080 rows for this volume's clamp
        sc = v.VScene(Camera=v.look_minus_x_camera(dist), DirectionalLight=base.DirectionalLight, Objects=[v.VVoxelObject(Volume=vol)],
                      EnvironmentMap=base.EnvironmentMap)
        p = v.default_params(480, 1080, vol.GetCellSize(), 255, shadow=True)
        p.cone_eps = math.tan(math.radians(30.0)) / 1080.0
        img, t = assert_parity(renderer, sc, p)
        assert t["hits"] > 0 and t["exhausted_rays"] == 0, dist


def test_sample_counters_do_not_carry_into_the_exhausted_count(renderer, oracle_lib):
    """17 overlapping instances of a volume no ray can hit or leave within the largest budget (65535 positions): every
    lane takes 17 x 65535 > 2^20 samples.  The sample counters report exactly that, the exhausted count exactly one per (ray,
    instance) — round 2 kept the exhausted count in the sample counters' upper 12 bits, which this overflows."""
    fog = v.VVoxelVolume(2, 100.0)
    fog.fill(lambda X, Y, Z: np.full_like(X, 1e-3))
    sc = v.VScene(Camera=v.look_minus_x_camera(300.0), DirectionalLight=v.demo_light(),
                  Objects=[v.VVoxelObject(Volume=fog) for _ in range(17)])
    p = v.default_params(8, 8, fog.GetCellSize(), 65535, shadow=False)
    p.eps_hit, p.step_min, p.cone_eps, p.k_relax, p.eps_in = 1e-4, 1e-4, 0.0, 1.0, 0.01
    img, t = gpu_render(renderer, sc, p)
    ref, st = OracleScene(sc).render(p, threads=8)
    # (36 of the 64 rays meet the volume box)
    assert t["primary_steps"] == st["primary_steps"] == 36 * 17 * 65535 and t["exhausted_rays"] == st["exhausted_rays"] == 36 * 17
    assert t["hits"] == st["hits"] == 0 and np.abs(img - ref).max() <= TOL


def _orbit(cam0, n):
    cams = []
    for f in range(n):
        a = 0.05 * f
        pos = (cam0.Position[0] * math.cos(a) - cam0.Position[1] * math.sin(a), cam0.Position[0] * math.sin(a) + cam0.Position[1] * math.cos(a),
               cam0.Position[2] + 1.5 * f)
        cams.append((pos, tuple(v.quat_mul(v.quat_from_axis_angle(v.UP, a), cam0.Rotation)), 60.0 - 0.25 * f))
    return cams


@pytest.mark.parametrize("case", ["lean", "bvh", "full", "lds", "cells16", "cube", "strips_rgba8"])
def test_fused_block_launch_equals_per_frame_launches(renderer, oracle_lib, case):
    """The march kernels' frame axis (vrt_render_block: ONE launch, blockIdx.y = frame, cameras in the kernarg segment or — more than
    MAX_BLOCK_FRAMES — in device memory) on every kernel family: a block of MAX_BLOCK_FRAMES + 3 frames is bit-equal to as many per-frame launches
    (VRT_FLAG_BLOCK_PER_FRAME), frame by frame; the counters vrt_last_timing reports are those of the block's last frame
    rendered alone; three of the frames against the oracle."""
    import copy
    import torch

    M = _abi.MAX_BLOCK_FRAMES
    n, W, H = M + 3, 136, 72
    path, mode, strips, rgba8 = _abi.PATH_AUTO, _abi.MODE_INTERP_NOTEX, None, False
    if case == "bvh":
        sc = scenes.config5_instances(5, 32)
    elif case == "full":
        sc = scenes.config3_torus(6, 32)
        sc.PointLights = [v.VPointLight(Position=(150.0, 40.0, 120.0), IlluminationStrength=400.0, Color=(1.0, 0.8, 0.6, 1.0),
                                        AttenuationLinear=0.05, AttenuationExp=0.002)]
    elif case == "cube":
        sc = scenes.config3_torus(5, 32)
        mode = _abi.MODE_CUBE_NOTEX
    else:
        sc = scenes.config3_voxelized(6, 16)
        if case == "lds":
            path = _abi.PATH_BRICK_LDS
        if case == "cells16":
            path = _abi.PATH_CELLS
            for vol in sc.volumes():
                vol.set_device_format(_abi.FORMAT_TEXEL16)
        if case == "strips_rgba8":
            strips, rgba8 = (8, 1, 3, 3), True  # rank 1 of 3: 72 rows = 9 strips of 8
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True, path=path)
    p.mode = mode
    if rgba8:
        p.flags |= _abi.FLAG_OUTPUT_RGBA8
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    cams = _orbit(sc.Camera, n)
    rows = strips[0] * strips[3] if strips else H
    shape, dt, bpp = (n, rows, W, 4), (torch.uint8 if rgba8 else torch.float32), (4 if rgba8 else 16)
    fused = torch.zeros(shape, dtype=dt, device="cuda:0")
    single = torch.zeros(shape, dtype=dt, device="cuda:0")
    kw = {"strips": strips} if strips else {"rows": (0, H)}
    renderer.render_block(p, n, fused.data_ptr(), rows * W * bpp, 0, cameras=cams, **kw)
    torch.cuda.synchronize()
    t_fused = renderer.last_timing()
    assert [fr for _, fr in renderer.launch_history(1)] == [n]  # more frames than the kernarg segment holds cameras: still ONE launch
    # ... and the block's first MAX_BLOCK_FRAMES frames alone (cameras in the kernarg segment): the same frames
    part = torch.zeros((M,) + shape[1:], dtype=dt, device="cuda:0")
    renderer.render_block(p, M, part.data_ptr(), rows * W * bpp, 0, cameras=cams[:M], **kw)
    torch.cuda.synchronize()
    assert [fr for _, fr in renderer.launch_history(1)] == [M] and torch.equal(part, fused[:M])
    pf = _abi.vrt_params.from_buffer_copy(p)
    pf.flags |= _abi.FLAG_BLOCK_PER_FRAME
    renderer.render_block(pf, n, single.data_ptr(), rows * W * bpp, 0, cameras=cams, **kw)
    torch.cuda.synchronize()
    t_single = renderer.last_timing()
    for f in range(n):
        assert torch.equal(fused[f], single[f]), (case, f)
    assert not torch.equal(fused[0], fused[n - 1])
    assert {k: t_fused[k] for k in STAT_KEYS} == {k: t_single[k] for k in STAT_KEYS} and t_fused["primary_rays"] == (rows if not strips else 24) * W
    if not strips:
        for f in (0, M - 1, n - 1):
            sf = copy.copy(sc)
            sf.Camera = v.VCamera(Position=cams[f][0], Rotation=cams[f][1], FOVAngle=cams[f][2])
            ref, _ = OracleScene(sf).render(p, threads=8)
            assert np.abs(fused[f].cpu().numpy() - ref).max() <= TOL, (case, f)


@pytest.mark.parametrize("case", ["demo_mirror", "demo_lean", "moving_lights", "one_instance", "changing_counts", "texel16_passes"])
def test_block_over_per_frame_scenes_equals_scene_set_per_frame(renderer, oracle_lib, case):
    """vrt_block::scenes: the reference moves objects every frame and rebuilds its TLAS every frame
    (RendererEngineInstance.cpp:111-130, DXRenderer.cpp:809-825); a block of frames over per-frame scene state — instances, BVH,
    lights, camera, cull rectangle per frame — is ONE march launch and renders every frame exactly as vrt_scene_set(frame's scene)
    + a one-frame launch does (pixels bit for bit, counters of the last frame), on the directional-light kernel, the full closest
    hit as one kernel and in passes, the single-instance kernels, frames whose instance / light counts differ; three frames
    against the oracle.  demo_*: the reference demo's own scene, its two spheres orbiting over 48 frames."""
    import copy
    import torch

    n, W, H = 48, 160, 90
    bounces = 0
    if case in ("demo_mirror", "demo_lean", "texel16_passes"):
        base = scenes.demo_scene(6, 16, mirror=(case != "demo_lean"))
        if case == "texel16_passes":
            for vol in base.volumes():
                vol.set_device_format(_abi.FORMAT_TEXEL16)
            base.PointLights = [v.VPointLight(Position=(250.0, 80.0, 200.0), IlluminationStrength=500.0, AttenuationLinear=0.02, AttenuationExp=0.001)]
        frames = scenes.demo_frames(base, n, dt=0.25)
        bounces = 2 if case != "demo_lean" else 0
    elif case == "moving_lights":
        base = scenes.full_closest_hit_scene(5, 16)
        frames = []
        for f in range(n):
            sc = copy.copy(base)
            a = 0.13 * f
            sc.PointLights = [copy.copy(base.PointLights[0])]
            sc.PointLights[0].Position = (150.0 * math.cos(a), 150.0 * math.sin(a), 120.0)
            sc.SpotLights = [copy.copy(base.SpotLights[0])] if f % 3 else []      # the spot light comes and goes
            sc.DirectionalLight = v.VLight(Rotation=tuple(v.quat_mul(v.quat_from_axis_angle(v.UP, 0.05 * f), base.DirectionalLight.Rotation)),
                                           IlluminationStrength=6.0 - 0.05 * f)
            sc.Camera = v.VCamera(Position=(420.0 - f, 2.0 * f, 40.0), Rotation=base.Camera.Rotation, FOVAngle=60.0)
            frames.append(sc)
        bounces = 1
    elif case == "one_instance":
        base = scenes.config3_voxelized(6, 16)
        frames = []
        for f in range(n):
            sc = copy.copy(base)
            o = copy.copy(base.Objects[0])
            o.Position = (3.0 * f - 40.0, 0.5 * f, 10.0 * math.sin(0.2 * f))
            o.Rotation = tuple(v.quat_from_axis_angle(v.UP, 0.04 * f))
            o.Scale = (1.0, 1.0 + 0.01 * f, 1.0)
            sc.Objects = [o]
            frames.append(sc)
    else:  # changing_counts: 0 .. 5 instances of two volumes, by frame
        base = scenes.config5_instances(5, 16, distinct_volumes=True)
        base.Objects = base.Objects[:5]
        frames = []
        for f in range(n):
            sc = copy.copy(base)
            sc.Objects = [copy.copy(o) for o in base.Objects[:f % 6]]
            for k, o in enumerate(sc.Objects):
                o.Position = (o.Position[0] + 4.0 * f * (k % 2), o.Position[1], o.Position[2] - 2.0 * f)
            frames.append(sc)
    p = v.default_params(W, H, scenes.min_cell(base), 255, shadow=True)
    p.max_bounces = bounces
    renderer.SetSceneToRender(base)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    arr = renderer.scene_array(frames)
    block = torch.zeros((n, H, W, 4), dtype=torch.float32, device="cuda:0")
    flag_sets = [0]
    if case in ("moving_lights", "texel16_passes"):
        flag_sets = [0, _abi.FLAG_FULL_ONE_KERNEL]  # the full closest hit of a block: in passes (default) and as one kernel
    outs = []
    for fl in flag_sets:
        q = _abi.vrt_params.from_buffer_copy(p)
        q.flags |= fl
        block.zero_()
        renderer.render_block(q, n, block.data_ptr(), H * W * 16, 0, scenes=(arr, 0))
        torch.cuda.synchronize()
        assert [fr for _, fr in renderer.launch_history(1)] == [n], "ONE launch for the block"
        t_block = renderer.last_timing()
        outs.append(block.clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    # the reference's way: the scene re-sent and one launch per frame
    one = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    lib = _abi.load()
    for f in range(n):
        _abi.check(lib.vrt_scene_set(renderer._ctx, C.byref(arr[f])), "vrt_scene_set")
        renderer.render_rows(p, 0, H, one.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(one, outs[0][f]), (case, f)
    t_one = renderer.last_timing()
    assert {k: t_block[k] for k in STAT_KEYS} == {k: t_one[k] for k in STAT_KEYS}
    assert not torch.equal(outs[0][0], outs[0][n - 1])
    for f in (0, n // 2, n - 1):
        ref, _ = OracleScene(frames[f]).render(p, threads=8)
        assert np.abs(outs[0][f].cpu().numpy() - ref).max() <= TOL, (case, f)
    renderer.SetSceneToRender(base)
    renderer.SyncWithScene()
    # a frame's scene that vrt_scene_set would refuse is refused here too; cameras next to scenes likewise
    bad = renderer.scene_array(frames[:2])
    bad[1].n_instances = 1
    bad[1].instances[0].volume_slot = 17
    with pytest.raises(RuntimeError):
        renderer.render_block(p, 2, block.data_ptr(), H * W * 16, 0, scenes=(bad, 0))
    with pytest.raises(RuntimeError):
        renderer.render_block(p, 2, block.data_ptr(), H * W * 16, 0, scenes=(arr, 0), cameras=_orbit(base.Camera, 2))


@pytest.mark.parametrize("full", [False, True])
def test_a_block_of_many_frames_is_one_launch(renderer, oracle_lib, full):
    """vrt_render_block with more frames than the kernarg segment holds cameras (here 130 and the maximum, 256): ONE launch with
    the camera records in device memory — the directional-light kernel and the full closest hit in passes —, bit-equal to per-frame
    launches; 257 frames are refused."""
    import torch

    sc = scenes.config3_torus(5, 16)
    if full:
        sc.PointLights = [v.VPointLight(Position=(150.0, 40.0, 120.0), IlluminationStrength=400.0, Color=(1.0, 0.8, 0.6, 1.0),
                                        AttenuationLinear=0.05, AttenuationExp=0.002)]
    W, H = 72, 40
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    for n in (130, _abi.MAX_LAUNCH_FRAMES):
        cams = _orbit(sc.Camera, n)
        fused = torch.zeros((n, H, W, 4), dtype=torch.float32, device="cuda:0")
        single = torch.zeros_like(fused)
        renderer.render_block(p, n, fused.data_ptr(), H * W * 16, 0, cameras=cams, rows=(0, H))
        torch.cuda.synchronize()
        assert [fr for _, fr in renderer.launch_history(1)] == [n]
        t_fused = renderer.last_timing()
        pf = _abi.vrt_params.from_buffer_copy(p)
        pf.flags |= _abi.FLAG_BLOCK_PER_FRAME
        renderer.render_block(pf, n, single.data_ptr(), H * W * 16, 0, cameras=cams, rows=(0, H))
        torch.cuda.synchronize()
        assert torch.equal(fused, single) and not torch.equal(fused[0], fused[n - 1])
        assert {k: t_fused[k] for k in STAT_KEYS} == {k: renderer.last_timing()[k] for k in STAT_KEYS}
    with pytest.raises(Exception):
        renderer.render_block(p, _abi.MAX_LAUNCH_FRAMES + 1, fused.data_ptr(), H * W * 16, 0, rows=(0, H))


def test_full_closest_hit_in_passes_on_two_streams_at_once(renderer, oracle_lib):
    """The passes of the full closest hit hand per-pixel hit records from one kernel to the next; every launch stream has its own
    (like the counters): two streams marching different blocks of a scene with a point light at the same time give the frames
    each gives alone, and those are the one-kernel form's (VRT_FLAG_FULL_ONE_KERNEL) bit for bit."""
    import torch

    sc = scenes.config3_torus(6, 32)
    sc.PointLights = [v.VPointLight(Position=(150.0, 40.0, 120.0), IlluminationStrength=400.0, Color=(1.0, 0.8, 0.6, 1.0),
                                    AttenuationLinear=0.05, AttenuationExp=0.002)]
    n, W, H = 12, 200, 120
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    cams = _orbit(sc.Camera, 2 * n)
    both = torch.zeros((2, n, H, W, 4), dtype=torch.float32, device="cuda:0")
    alone = torch.zeros_like(both)
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(3):  # several rounds, so that the two streams' launches do overlap
        for i, st in enumerate(streams):
            renderer.render_block(p, n, both[i].data_ptr(), H * W * 16, st.cuda_stream, cameras=cams[i * n:(i + 1) * n], rows=(0, H))
    torch.cuda.synchronize()
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= _abi.FLAG_FULL_ONE_KERNEL
    for i in range(2):
        renderer.render_block(q, n, alone[i].data_ptr(), H * W * 16, 0, cameras=cams[i * n:(i + 1) * n], rows=(0, H))
        torch.cuda.synchronize()
    assert torch.equal(both, alone) and not torch.equal(both[0], both[1])
    assert float(both[..., :3].max()) > 0.2


def test_full_closest_hit_in_passes_can_be_captured_into_a_graph(renderer, oracle_lib):
    """A block of frames of a scene with lights AND a mirroring material — three kernels per launch: camera-ray pass, light pass,
    the bouncing lanes' pass — captured into a HIP graph after one warm launch of that size on the stream (which allocates the hit
    records), replayed: the direct launch's frames; a later, larger launch on the stream retires the records, never frees them."""
    import torch

    sc = scenes.full_closest_hit_scene(5, 16)
    n, W, H = 4, 160, 96
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    p.max_bounces = 2
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    cams = _orbit(sc.Camera, n)
    side = torch.cuda.Stream()
    direct = torch.zeros((n, H, W, 4), dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(side):
        renderer.render_block(p, n, direct.data_ptr(), H * W * 16, side.cuda_stream, cameras=cams, rows=(0, H))
    torch.cuda.synchronize()
    t_direct = renderer.last_timing()
    assert t_direct["bounce_rays"] > 0 and t_direct["shadow_rays"] > 0
    out = torch.zeros_like(direct)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        renderer.render_block(p, n, out.data_ptr(), H * W * 16, side.cuda_stream, cameras=cams, rows=(0, H))
    assert float(out.abs().max()) == 0.0
    for rep in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, direct)
        if rep == 0:  # a larger block on the same stream: its hit records outgrow the captured launch's
            bigger = torch.zeros((2 * n, H, W, 4), dtype=torch.float32, device="cuda:0")
            with torch.cuda.stream(side):
                renderer.render_block(p, 2 * n, bigger.data_ptr(), H * W * 16, side.cuda_stream, cameras=_orbit(sc.Camera, 2 * n), rows=(0, H))
            torch.cuda.synchronize()
            assert torch.equal(bigger[:n], direct)
    q = _abi.vrt_params.from_buffer_copy(p)
    q.flags |= _abi.FLAG_FULL_ONE_KERNEL
    one = torch.zeros_like(direct)
    renderer.render_block(q, n, one.data_ptr(), H * W * 16, 0, cameras=cams, rows=(0, H))
    torch.cuda.synchronize()
    assert torch.equal(one, direct) and {k: renderer.last_timing()[k] for k in STAT_KEYS} == {k: t_direct[k] for k in STAT_KEYS}


@pytest.mark.parametrize("seed", range(96))
def test_random_scenes_parity(oracle_lib, seed):
    """Fuzz: seeded random scenes (instances with arbitrary rotations and anisotropic / mirrored scales, shell and SDF
    volumes, lights, textures, every render mode, bounces, tight budgets) through the C-ABI against the oracle:
    <= 1e-4 per channel, ray and hit counters exact (sample counters too when there is one instance: with several,
    the BVH visits instances in a different order than the oracle's loop and prunes differently)."""
    sc, p = scenes.random_scene(seed)
    r = v.VHipRenderer()
    assert r.Start()
    try:
        img, t = gpu_render(r, sc, p)
        # the full closest hit's three-pass form (what a block of frames runs; a scene without extra lights, bounces or textures
        # never runs it and renders the same way twice): the same bits and the same counters as the one kernel
        p3 = _abi.vrt_params.from_buffer_copy(p)
        p3.flags |= _abi.FLAG_FULL_THREE_PASS
        img3, t3 = gpu_render(r, sc, p3)
    finally:
        r.Stop()
    assert np.array_equal(img, img3), f"seed {seed}: three-pass form differs in {np.count_nonzero(img != img3)} values"
    assert {k: t[k] for k in STAT_KEYS} == {k: t3[k] for k in STAT_KEYS}, f"seed {seed}"
    ref, st = OracleScene(sc).render(p, threads=8)
    assert not np.isnan(img).any()
    err = np.abs(img - ref)
    assert err.max() <= TOL, f"seed {seed}: max abs err {err.max()} at {np.unravel_index(err.argmax(), err.shape)} mode {p.mode}"
    keys = STAT_KEYS if len(sc.Objects) == 1 else ("primary_rays", "shadow_rays", "bounce_rays", "hits")
    assert {k: t[k] for k in keys} == {k: st[k] for k in keys}, f"seed {seed}"


@pytest.mark.parametrize("seed", range(200, 248))
def test_random_scenes_parity_with_the_reference_switches(oracle_lib, seed):
    """The fuzz scenes again (other seeds) with what the C++ adaptor switches on by default: both reference-artefact flags, and the material
    slots a seed leaves unbound filled with 1x1 CONSTANT textures (the reference's default normal texel; for every third seed a constant
    albedo / RM texel too) next to whatever images the seed bound — constants and images mix in one material, the lean kernel's REF
    instantiation, the BVH form, the Cube modes, the passes and the full kernel all see the switches.  GPU = oracle <= 1e-4, counters exact."""
    sc, p = scenes.random_scene(seed)
    for k, vol in enumerate(sc.volumes()):
        m = vol.Material
        if m.NormalTexture is None:
            m.NormalTexture = scenes.reference_default_normal_texel()
        if (seed + k) % 3 == 0:
            if m.AlbedoTexture is None:
                m.AlbedoTexture = np.array([[[250 - 9 * k, 200, 120 + 7 * k, 255]]], np.uint8)
            if m.RMTexture is None:
                m.RMTexture = np.array([[[255 - 40 * (seed % 5), 128, 0, 255]]], np.uint8)
    p.flags |= REF_FLAGS
    r = v.VHipRenderer()
    assert r.Start()
    try:
        img, t = gpu_render(r, sc, p)
        p3 = _abi.vrt_params.from_buffer_copy(p)
        p3.flags |= _abi.FLAG_FULL_THREE_PASS
        img3, t3 = gpu_render(r, sc, p3)
    finally:
        r.Stop()
    assert np.array_equal(img, img3) and {k: t[k] for k in STAT_KEYS} == {k: t3[k] for k in STAT_KEYS}, f"seed {seed}"
    ref, st = OracleScene(sc).render(p, threads=8)
    assert not np.isnan(img).any()
    err = np.abs(img - ref)
    assert err.max() <= TOL, f"seed {seed}: max abs err {err.max()} at {np.unravel_index(err.argmax(), err.shape)} mode {p.mode}"
    keys = STAT_KEYS if len(sc.Objects) == 1 else ("primary_rays", "shadow_rays", "bounce_rays", "hits")
    assert {k: t[k] for k in keys} == {k: st[k] for k in keys}, f"seed {seed}"


@pytest.mark.parametrize("seed", [5018, 8081, 13831, 14789])
def test_specular_highlight_pixels_found_by_the_soak(oracle_lib, seed):
    """Four scenes of tests/soak_random_scenes.py (26 000 seeds) in which ONE pixel was 1.4e-4 ... 4e-4 off: a dark channel of
    a specular highlight on a smooth material, where c = (n.h)^2 (a^2 - 1) + 1 cancels to 1e-3 and the half vector's 1-ulp
    hardware reciprocal square root became 2e-4 of the distribution term.  With the correctly rounded one they sit at 1e-6."""
    sc, p = scenes.random_scene(seed)
    if seed != 5018:  # the soak's "mix" draw for these seeds
        rng = np.random.RandomState(seed + 77777)
        p.path = int(rng.choice([_abi.PATH_AUTO, _abi.PATH_DENSE, _abi.PATH_BRICK, _abi.PATH_BRICK_LDS, _abi.PATH_CELLS]))
        fmt = int(rng.choice([_abi.FORMAT_F32, _abi.FORMAT_TEXEL16]))
        p.k_relax = float(rng.choice([0.7, 1.0, 1.4, 1.7, 2.0]))
        for vol in sc.volumes():
            vol.set_device_format(fmt)
    r = v.VHipRenderer()
    assert r.Start()
    try:
        img, t = gpu_render(r, sc, p)
    finally:
        r.Stop()
    ref, st = OracleScene(sc).render(p, threads=8)
    assert np.abs(img - ref).max() <= 1e-5
    assert t["hits"] == st["hits"] and t["shadow_rays"] == st["shadow_rays"]


def test_multi_tile_context_on_one_gpu(oracle_lib):
    """A context with three logical devices (the same ordinal three times) exercises the interleaved-strip split and the
    peer gather into device 0's frame that an 8-GPU context uses: one strip per device with a ragged last one (90 rows),
    and several strips per device with an empty strip slot on the last device (230 rows = 8 strips over 3 devices)."""
    sc = scenes.config5_instances(5, 16)
    r2 = v.VHipRenderer(devices=(0, 0, 0))
    assert r2.Start()
    try:
        for w, h in ((96, 230), (160, 90)):
            p = v.default_params(w, h, scenes.min_cell(sc), 255, shadow=True)
            img, t = gpu_render(r2, sc, p)
            ref, st = OracleScene(sc).render(p, threads=8)
            assert np.abs(img - ref).max() <= TOL
            assert t["primary_rays"] == w * h and t["hits"] == st["hits"]
        q = _abi.vrt_params.from_buffer_copy(p)
        q.flags |= _abi.FLAG_OUTPUT_RGBA8  # the 4-byte tiles take the same split + peer gather
        img8, _ = gpu_render(r2, sc, q)
        from test_tiles_gloo import quantize_rgba8
        assert img8.dtype == np.uint8 and np.array_equal(img8, quantize_rgba8(img))
        # the benchmark's frame size: 1920x1080 = 135 strips of 8 rows over 3 devices, bit-equal to the one-device frame
        big = v.default_params(1920, 1080, scenes.min_cell(sc), 255, shadow=True)
        split, ts = gpu_render(r2, sc, big)
        r1 = v.VHipRenderer()
        assert r1.Start()
        try:
            whole, tw = gpu_render(r1, sc, big)
        finally:
            r1.Stop()
        assert np.array_equal(split, whole) and ts["hits"] == tw["hits"] and ts["primary_rays"] == 1920 * 1080
        assert _oracle_bands(sc, big, split, bands=4) <= TOL
    finally:
        r2.Stop()


def test_voxel_record_upload_and_volume_lifecycle(renderer, oracle_lib):
    lib = _abi.load()
    sc = scenes.config2_sphere(5, 8)
    p = v.default_params(96, 54, scenes.min_cell(sc), 128, shadow=True)
    ref, _ = OracleScene(sc).render(p, threads=4)
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(96, 54)
    renderer.params_override = p
    renderer.SetRendererMode(p.mode)
    renderer.SyncWithScene()
    vol = sc.volumes()[0]
    renderer.upload_volume(0, vol, as_voxels=True)  # straight from VVoxel records
    img = renderer.Render()
    assert np.abs(img - ref).max() <= TOL
    ctx = renderer._ctx
    assert lib.vrt_volume_free(ctx, 7) == _abi.VRT_ERR_SLOT
    assert lib.vrt_volume_free(ctx, 99) == _abi.VRT_ERR_SLOT
    assert lib.vrt_volume_upload(ctx, 25, 3, 1.0, None, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_free(ctx, 0) == _abi.VRT_OK
    pp = renderer.make_params()
    assert lib.vrt_render(ctx, C.byref(pp), None) == _abi.VRT_ERR_NOT_READY  # scene referenced the freed slot
    renderer._uploaded.clear()
    img = renderer.Render()  # re-sync uploads again
    assert np.abs(img - ref).max() <= TOL


def test_full_size_properties_1080p_256(renderer):
    """BASELINE size (1920x1080, 256^3): size-independent properties instead of a CPU re-run —
    determinism, row-tile seamlessness, unlit pixels ∈ {tone-mapped tint, environment}, and the
    image symmetry of a symmetric scene."""
    import torch

    sc = scenes.config3_torus(8, 64)
    sc.Camera = v.look_minus_x_camera(320.0)  # torus around Z seen edge-on: mirror-symmetric in image y ↔ -y
    p = v.default_params(1920, 1080, scenes.min_cell(sc), 255, shadow=False, mode=_abi.MODE_INTERP_NOTEX_UNLIT)
    a, t = gpu_render(renderer, sc, p)
    b, _ = gpu_render(renderer, sc, p)
    assert np.array_equal(a, b)
    assert t["primary_rays"] == 1920 * 1080 and t["hits"] > 50000
    tint = np.array(sc.Objects[0].Volume.Material.AlbedoColor[:3], dtype=np.float32)
    tm = (tint / (tint + 1)) ** (1 / 2.2)
    hit = np.abs(a[..., :3] - tm).max(-1) < 1e-5
    assert hit.sum() == t["hits"]
    # hit mask is symmetric under a vertical flip (camera on the torus' symmetry plane)
    assert (hit != hit[::-1]).sum() <= 0.002 * hit.sum()
    full = torch.empty((1080, 1920, 4), dtype=torch.float32, device="cuda:0")
    for g in range(8):
        renderer.render_rows(p, g * 135, 135, full[g * 135:(g + 1) * 135].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(full.cpu().numpy(), a)


@pytest.mark.parametrize("path", [_abi.PATH_BRICK, _abi.PATH_DENSE, _abi.PATH_BRICK_LDS])
def test_voxelized_shell_volume_parity(renderer, oracle_lib, path):
    """BASELINE config 3 proper: a triangle mesh through the C++ Voxelizer (unsigned shell field,
    density_scale = thr, step_max = thr/2), rendered with the shadow ray on."""
    sc = scenes.config3_voxelized(6, 32)
    p = v.default_params(480, 270, scenes.min_cell(sc), 255, shadow=True, path=path)
    img, t = assert_parity(renderer, sc, p)
    assert (t["primary_steps"] + t["shadow_steps"]) / t["hits"] > 5 and t["hits"] > 10000


def test_bgra8_output_is_the_rgba8_frame_with_red_and_blue_swapped(renderer, oracle_lib):
    """VRT_FLAG_OUTPUT_BGRA8: the reference's back buffer is DXGI_FORMAT_B8G8R8A8_UNORM (DXConstants.cpp:21,
    DXRenderer.cpp:1322).  Same 8-bit values as the R8G8B8A8 target, B in the low byte — lean kernel, full closest hit (one kernel and
    passes), block launch; the flag alone (without RGBA8) is refused."""
    import torch

    for sc, bounces in ((scenes.config3_voxelized(6, 16), 0), (scenes.full_closest_hit_scene(5, 16), 2)):
        p = v.default_params(200, 112, scenes.min_cell(sc), 255, shadow=True)
        p.max_bounces = bounces
        p.flags |= _abi.FLAG_OUTPUT_RGBA8
        rgba, _ = gpu_render(renderer, sc, p)
        q = _abi.vrt_params.from_buffer_copy(p)
        q.flags |= _abi.FLAG_OUTPUT_BGRA8
        bgra, _ = gpu_render(renderer, sc, q)
        assert np.array_equal(bgra[..., [2, 1, 0, 3]], rgba) and (rgba[..., 3] == 255).all() and not np.array_equal(bgra, rgba)
        n = 3
        blk = torch.zeros((n, 112, 200, 4), dtype=torch.uint8, device="cuda:0")
        renderer.render_block(q, n, blk.data_ptr(), 112 * 200 * 4, 0, cameras=_orbit(sc.Camera, n))
        torch.cuda.synchronize()
        ref = torch.zeros_like(blk)
        renderer.render_block(p, n, ref.data_ptr(), 112 * 200 * 4, 0, cameras=_orbit(sc.Camera, n))
        torch.cuda.synchronize()
        assert torch.equal(blk[..., [2, 1, 0, 3]], ref)
    only = _abi.vrt_params.from_buffer_copy(p)
    only.flags = _abi.FLAG_OUTPUT_BGRA8
    one = torch.zeros((112, 200, 4), dtype=torch.float32, device="cuda:0")
    assert _abi.load().vrt_render_rows(renderer._ctx, C.byref(only), 0, 112, C.c_void_p(one.data_ptr()), None) == _abi.VRT_ERR_INVALID


def test_render_block_host_hands_the_frames_to_the_host(renderer, oracle_lib):
    """vrt_render_block_host: the block launch for callers without device memory (the C++ adaptor's RenderBlock): frames in
    context-owned pinned memory, bit-equal to vrt_render_block's — a camera path of 70 frames (copied in parts under the march) and
    a block over per-frame scenes."""
    import torch

    sc = scenes.config3_voxelized(6, 16)
    W, H, n = 168, 96, 70
    p = v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)
    p.flags |= _abi.FLAG_OUTPUT_RGBA8 | _abi.FLAG_OUTPUT_BGRA8
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    cams = renderer.camera_array(_orbit(sc.Camera, n))
    dev = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda:0")
    renderer.render_block(p, n, dev.data_ptr(), H * W * 4, 0, cameras=(cams, 0))
    torch.cuda.synchronize()
    b = _abi.vrt_block()
    b.n_frames, b.rows = n, H
    b.cameras = C.cast(cams, C.POINTER(_abi.vrt_camera))
    ptr = C.c_void_p()
    lib = _abi.load()
    _abi.check(lib.vrt_render_block_host(renderer._ctx, C.byref(p), C.byref(b), C.byref(ptr)), "vrt_render_block_host")
    host = np.frombuffer((C.c_uint8 * (n * H * W * 4)).from_address(ptr.value), dtype=np.uint8).reshape(n, H, W, 4)
    assert np.array_equal(host, dev.cpu().numpy())
    frames = scenes.moving_instances(sc, 9)
    arr = renderer.scene_array(frames)
    dev9 = torch.zeros((9, H, W, 4), dtype=torch.uint8, device="cuda:0")
    renderer.render_block(p, 9, dev9.data_ptr(), H * W * 4, 0, scenes=(arr, 0))
    torch.cuda.synchronize()
    b2 = _abi.vrt_block()
    b2.n_frames, b2.rows = 9, H
    b2.scenes = C.cast(arr, C.POINTER(_abi.vrt_scene))
    _abi.check(lib.vrt_render_block_host(renderer._ctx, C.byref(p), C.byref(b2), C.byref(ptr)), "vrt_render_block_host")
    host9 = np.frombuffer((C.c_uint8 * (9 * H * W * 4)).from_address(ptr.value), dtype=np.uint8).reshape(9, H, W, 4)
    assert np.array_equal(host9, dev9.cpu().numpy()) and not np.array_equal(host9[0], host9[8])
    assert lib.vrt_render_block_host(renderer._ctx, C.byref(p), C.byref(b2), None) == _abi.VRT_ERR_INVALID


def test_cpp_host_adaptor_block_of_the_demo_animation_equals_frame_by_frame(tmp_path):
    """VHipRenderer::RenderBlock (the VRenderer-shaped side of vrt_block::scenes): the demo's animation — its two spheres orbiting —
    as ONE march launch per 12 frames writes the same last frame as 12 Render() calls with three frames in flight and as 12
    synchronous ones, in every frame format (the PPM holds R, G, B whatever the byte order in memory)."""
    import subprocess

    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    outs = {}
    for name, extra in (("block_bgra8", ["--block", "12"]), ("flight_bgra8", []), ("sync_rgba8", ["--in-flight", "1", "--format", "rgba8"]),
                        ("sync_float", ["--in-flight", "1", "--format", "float"]), ("block_float", ["--block", "5", "--format", "float"])):
        out = str(tmp_path / (name + ".ppm"))
        r = subprocess.run([exe, "--frames", "12", "--size", "320x180", "--out", out] + extra, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr
        outs[name] = open(out, "rb").read()
    assert len(set(outs.values())) == 1, {k: len(x) for k, x in outs.items()}


REFERENCE_DEFAULT_NORMAL_TEXEL = np.array([[[127, 127, 255, 255]]], np.uint8)  # VColor(0.5, 0.5, 1, 1) * 255, truncated (DXTexture2D.cpp:63-71)


def test_cpp_host_adaptor_renders_the_demo_scene(renderer, tmp_path):
    """The C++ VRenderer adaptor (csrc/host/HipRenderer.cpp, driven by vrt_demo exactly like
    VEngine::EngineLoop drives the reference's renderer) against the Python host path on the same
    scene: App/Private/RendererEngineInstance.cpp:232-316 at frame 0."""
    import subprocess

    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out = str(tmp_path / "demo.ppm")
    r = subprocess.run([exe, "--frames", "1", "--size", "320x180", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    ppm = np.frombuffer(raw[raw.index(b"255\n") + 4:], dtype=np.uint8).reshape(180, 320, 3)

    mat = lambda c: v.VMaterial(c, 0.1, 0.6)
    S = 256
    tint = np.array([[1, .85, .8], [.8, .85, 1], [.85, 1, .8], [1, .8, 1], [.6, .75, 1], [.55, .5, .45]], np.float32)
    g = (0.35 + 0.6 * (1.0 - (np.arange(S, dtype=np.float32) + 0.5) / S)).astype(np.float32)
    env = np.zeros((6, S, S, 4), np.uint8)
    for f in range(6):
        env[f, :, :, :3] = np.minimum(255.0, g[:, None, None] * tint[f][None, None, :] * 255.0 + 0.5).astype(np.uint8)
    env[..., 3] = 255
    sc = v.VScene(Camera=v.VCamera(Position=(300.0, 0.0, 100.0), Rotation=tuple(v.quat_from_axis_angle(v.UP, 3.14159265))),
                  DirectionalLight=v.demo_light(),
                  Objects=[v.VVoxelObject(Position=(200.0, 0.0, 100.0), Volume=v.sphere_volume(6, 100.0, 40.0, mat((1, 0, 0, 1)))),
                           v.VVoxelObject(Position=(100.0, 0.0, 200.0), Volume=v.sphere_volume(6, 100.0, 20.0, mat((0, 0, 1, 1))))],
                  EnvironmentMap=env)
    for vol in sc.volumes():
        vol.set_device_format(_abi.FORMAT_TEXEL16)  # the C++ adaptor's default: the reference's own volume texel
        # ... and the reference's 1x1 default normal texel (127, 127, 255) on materials without a normal map (RDXScene.cpp:241-260),
        # which the adaptor binds by default: in Interp, the reference's default mode, it tilts every normal by 0.3 degrees
        vol.Material.NormalTexture = REFERENCE_DEFAULT_NORMAL_TEXEL
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(320, 180)
    renderer.params_override = None
    renderer.MaxSteps, renderer.Shadows, renderer.DataPath = 255, True, _abi.PATH_AUTO
    renderer.ReferenceViewVector = renderer.ReferenceBoundaryTexels = True  # ... and its two reference-artefact flags (round 5)
    renderer.SetRendererMode(_abi.MODE_INTERP)
    try:
        img = renderer.Render()
    finally:
        renderer.ReferenceViewVector = renderer.ReferenceBoundaryTexels = False
    py8 = (np.clip(img[..., :3], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    diff = np.abs(py8.astype(int) - ppm.astype(int))
    # identical pipeline up to the light quaternion's last bit (float sin/cos vs double) and 8-bit rounding
    assert (diff > 1).mean() < 2e-3, f"{(diff > 1).sum()} pixels differ by more than one 8-bit step"
    assert (ppm[..., 0].astype(int) - ppm[..., 2] > 60).sum() > 2000  # the red sphere is in the frame
    # --identity-defaults: unbound slots are exact identities — the NoTex frame — and the default texel's 0.3-degree tilt is visible against it
    out2 = str(tmp_path / "demo_identity.ppm")
    r = subprocess.run([exe, "--frames", "1", "--size", "320x180", "--out", out2, "--identity-defaults"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw2 = open(out2, "rb").read()
    ppm2 = np.frombuffer(raw2[raw2.index(b"255\n") + 4:], dtype=np.uint8).reshape(180, 320, 3)
    for vol in sc.volumes():
        vol.Material.NormalTexture = None
    renderer.SetRendererMode(_abi.MODE_INTERP_NOTEX)
    plain8 = (np.clip(renderer.Render()[..., :3], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert (np.abs(plain8.astype(int) - ppm2.astype(int)) > 1).mean() < 2e-3
    assert 0.005 < (np.abs(ppm2.astype(int) - ppm.astype(int)) > 1).mean() < 0.2


def test_cpp_host_adaptor_binds_material_textures_from_a_vox_scene(renderer, tmp_path):
    """A .vox scene whose material names texture files (VMaterial::AlbedoTexturePath / RMTexturePath, Material.h:29-31):
    the C++ adaptor resolves the paths (a PNG and a binary PPM here; the reference decodes with WIC/DDS), uploads them through
    vrt_texture_upload and binds them with vrt_volume_set_textures.  Same frame as the Python host with the same images."""
    import subprocess

    from volumetricraytracer_amd import vox_io

    alb, _, rm = scenes.procedural_textures()

    def write_ppm(path, img):
        with open(path, "wb") as f:
            f.write(b"P6\n# material texture\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
            f.write(np.ascontiguousarray(img[..., :3]).tobytes())

    from test_voxelizer import _write_png

    alb_path, rm_path = str(tmp_path / "albedo.png"), str(tmp_path / "rm.ppm")
    _write_png(alb_path, alb[..., :3], 2)  # one texture through the PNG decoder, one through the PPM reader
    write_ppm(rm_path, rm)
    rm_rgb = rm.copy()
    rm_rgb[..., 3] = 255
    torus = v.torus_volume(6, 100.0, 60.0, 25.0, v.VMaterial((0.9, 0.9, 0.9, 1.0), 0.9, 0.5, AlbedoTexturePath=alb_path, RMTexturePath=rm_path,
                                                              TextureScale=(30.0, 45.0)))
    obj = v.VVoxelObject(Position=(60.0, 0.0, 60.0), Rotation=tuple(v.quat_from_axis_angle(v.RIGHT, 0.7)), Volume=torus)
    vox = str(tmp_path / "scene.vox")
    vox_io.save_scene(v.VScene(Objects=[obj], DirectionalLight=v.demo_light()), vox)  # the file's light is the one the demo keeps
    exe = os.path.join(os.path.dirname(_abi.LIB_PATH), "vrt_demo")
    out = str(tmp_path / "demo.ppm")
    r = subprocess.run([exe, "--frames", "1", "--size", "320x180", "--scene", vox, "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "left unbound" not in r.stderr, r.stderr
    raw = open(out, "rb").read()
    ppm = np.frombuffer(raw[raw.index(b"255\n") + 4:], dtype=np.uint8).reshape(180, 320, 3)

    torus.Material.AlbedoTexture, torus.Material.RMTexture = alb, rm_rgb
    mat = lambda c: v.VMaterial(c, 0.1, 0.6)
    S = 256
    tint = np.array([[1, .85, .8], [.8, .85, 1], [.85, 1, .8], [1, .8, 1], [.6, .75, 1], [.55, .5, .45]], np.float32)
    g = (0.35 + 0.6 * (1.0 - (np.arange(S, dtype=np.float32) + 0.5) / S)).astype(np.float32)
    env = np.zeros((6, S, S, 4), np.uint8)
    for f in range(6):
        env[f, :, :, :3] = np.minimum(255.0, g[:, None, None] * tint[f][None, None, :] * 255.0 + 0.5).astype(np.uint8)
    env[..., 3] = 255
    sc = v.VScene(Camera=v.VCamera(Position=(300.0, 0.0, 100.0), Rotation=tuple(v.quat_from_axis_angle(v.UP, 3.14159265))),
                  DirectionalLight=v.demo_light(),
                  Objects=[obj,
                           v.VVoxelObject(Position=(200.0, 0.0, 100.0), Volume=v.sphere_volume(6, 100.0, 40.0, mat((1, 0, 0, 1)))),
                           v.VVoxelObject(Position=(100.0, 0.0, 200.0), Volume=v.sphere_volume(6, 100.0, 20.0, mat((0, 0, 1, 1))))],
                  EnvironmentMap=env)
    for vol in sc.volumes():
        vol.set_device_format(_abi.FORMAT_TEXEL16)  # the C++ adaptor's default
        if vol.Material.NormalTexture is None:
            vol.Material.NormalTexture = REFERENCE_DEFAULT_NORMAL_TEXEL  # what the adaptor binds to a material without a normal map
    r2 = v.VHipRenderer()
    assert r2.Start()
    try:
        r2.SetSceneToRender(sc)
        r2.ResizeRenderOutput(320, 180)
        r2.SetRendererMode(_abi.MODE_INTERP)
        r2.ReferenceViewVector = r2.ReferenceBoundaryTexels = True  # the adaptor's defaults (round 5)
        img = r2.Render()
        r2.SetRendererMode(_abi.MODE_INTERP_NOTEX)
        plain = r2.Render()
    finally:
        r2.Stop()
    py8 = (np.clip(img[..., :3], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    diff = np.abs(py8.astype(int) - ppm.astype(int))
    assert (diff > 1).mean() < 2e-3, f"{(diff > 1).sum()} pixels differ by more than one 8-bit step"
    assert np.abs(img - plain).max() > 0.1  # the textures are really in the frame


@pytest.mark.parametrize("bounces", [0, 1, 2])
@pytest.mark.parametrize("path", [_abi.PATH_BRICK, _abi.PATH_DENSE])
def test_full_closest_hit_parity(renderer, oracle_lib, bounces, path):
    """point + spot lights with their own shadow rays and the mirror bounce down to
    MAX_RAY_RECURSION_DEPTH, against the (recursive) oracle."""
    sc = scenes.full_closest_hit_scene(6, 32)
    p = v.default_params(480, 270, scenes.min_cell(sc), 255, shadow=True, path=path)
    p.max_bounces = bounces
    img, t = assert_parity(renderer, sc, p, check_stats=False)
    ref, st = OracleScene(sc).render(p, threads=8)
    for key in ("hits", "shadow_rays", "bounce_rays", "primary_rays"):
        assert t[key] == st[key], key
    assert (st["bounce_rays"] > 1000) == (bounces > 0)


def test_full_closest_hit_single_instance_counters(renderer, oracle_lib):
    vol = v.sphere_volume(6, 100.0, 60.0, v.VMaterial((0.9, 0.6, 0.3, 1.0), 0.1, 0.6))
    sc = scenes.full_closest_hit_scene(5, 16)
    sc.Objects = [v.VVoxelObject(Volume=vol)]
    sc.Camera = v.look_minus_x_camera(260.0)
    p = v.default_params(320, 180, vol.GetCellSize(), 255, shadow=True)
    p.max_bounces = 2
    assert_parity(renderer, sc, p, check_stats=True)
