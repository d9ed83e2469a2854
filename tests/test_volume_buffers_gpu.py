"""Every device buffer of a volume slot (vrt_debug_volume_bytes: dense grid, materials, bricks, cell records, both levels of the
empty-space table, the Cube table, the active box) against the plain-numpy reference of tests/volume_ref.py, byte for byte: every
upload path, both formats, resolutions 0 .. 9, bounded and unbounded metrics, several devices, region edits and non-finite
densities."""
import ctypes as C

import numpy as np
import pytest

import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import workloads as scenes
from oracle.binding import OracleScene
from test_volume_edit_gpu import edit_sequence, update

pytestmark = pytest.mark.gpu
TOL = 1e-4
STAT_KEYS = ("primary_rays", "shadow_rays", "bounce_rays", "primary_steps", "shadow_steps", "hits", "exhausted_rays")
WHICH = {"dense": _abi.VOLUME_BYTES_DENSE, "material": _abi.VOLUME_BYTES_MATERIAL, "bricks": _abi.VOLUME_BYTES_BRICKS,
         "cells": _abi.VOLUME_BYTES_CELLS, "skip": _abi.VOLUME_BYTES_SKIP, "nib": _abi.VOLUME_BYTES_NIB,
         "cube_skip": _abi.VOLUME_BYTES_CUBE_SKIP, "active_box": _abi.VOLUME_BYTES_ACTIVE_BOX}
F32, T16 = _abi.FORMAT_F32, _abi.FORMAT_TEXEL16


def read(r, slot, name, device=0) -> np.ndarray:
    size = C.c_size_t(0)
    _abi.check(r._lib.vrt_debug_volume_bytes(r._ctx, slot, device, WHICH[name], None, 0, C.byref(size)), "vrt_debug_volume_bytes")
    buf = np.zeros(size.value, np.uint8)
    _abi.check(r._lib.vrt_debug_volume_bytes(r._ctx, slot, device, WHICH[name], buf.ctypes.data_as(C.c_void_p), buf.size,
                                             C.byref(size)), "vrt_debug_volume_bytes")
    return buf


def assert_bytes(got: np.ndarray, want: np.ndarray, what: str):
    assert got.size == want.size, f"{what}: {got.size} bytes, want {want.size}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{what}: {bad.size} of {got.size} bytes differ, first at byte {bad[0]} (got {got[bad[0]]}, want {want[bad[0]]})")


def check_slot(r, slot, want: dict, what: str, devices=(0,)):
    """Every buffer of the slot on every device equals the reference (the active box only where the slot has tables)."""
    for dev in devices:
        for name, ref in want.items():
            if ref is None:
                continue
            assert_bytes(read(r, slot, name, dev), ref, f"{what}: device {dev} buffer {name}")


def set_metric(r, slot, scale, step):
    _abi.check(r._lib.vrt_volume_set_metric(r._ctx, slot, float(scale), float(step)), "vrt_volume_set_metric")


def upload(r, slot, vol, fmt, path):
    """Uploads vol by `path` ('float', 'float_nomat', 'voxels', 'texels'); returns the (dense, material) the slot must hold."""
    lib, ctx = r._lib, r._ctx
    _abi.check(lib.vrt_set_volume_format(ctx, fmt), "vrt_set_volume_format")
    d = np.ascontiguousarray(vol.density, np.float32)
    m = np.ascontiguousarray(vol.material_id, np.uint8)
    if path == "texels":
        tex = vol.reference_texels()
        rc = lib.vrt_volume_upload_texels(ctx, slot, vol.Resolution, vol.VolumeExtends, tex.ctypes.data_as(C.c_void_p))
        want = R.decode_texels(tex)
    elif path == "voxels":
        rec = vol.voxel_records()
        rc = lib.vrt_volume_upload_voxels(ctx, slot, vol.Resolution, vol.VolumeExtends, rec.ctypes.data_as(C.c_void_p))
        dens, mat = R.split_records(rec)
        want = (R.dense_field(dens.reshape(d.shape), fmt), mat.reshape(d.shape))
    else:
        nomat = path == "float_nomat"
        rc = lib.vrt_volume_upload(ctx, slot, vol.Resolution, vol.VolumeExtends, d.ctypes.data_as(C.c_void_p),
                                   None if nomat else m.ctypes.data_as(C.c_void_p))
        want = (R.dense_field(d, fmt), np.zeros_like(m) if nomat else m)
    _abi.check(rc, "vrt_volume_upload*")
    return want


class RefCache:
    """device_bytes of one DENSE field under several metrics, each computed once; the dense / material entries per upload."""

    def __init__(self, dense, fmt, which=None):
        self.dense, self.fmt, self.which, self.tabs = np.ascontiguousarray(dense, np.float32), fmt, which, {}

    def want(self, material, scale, step):
        key = (float(np.float32(scale)), float(np.float32(step)) if step > 0 else 0.0)
        if key not in self.tabs:
            self.tabs[key] = R.device_bytes(self.dense, material, self.fmt, scale, step, self.which)
        out = dict(self.tabs[key])
        out["material"] = np.ascontiguousarray(material, np.uint8).reshape(-1)
        return out


def sample_volume(res):
    """Sphere with a material byte pattern: every byte of the material buffer is checked."""
    vol = v.sphere_volume(res, 100.0, 40.0)
    vol.material_id = ((np.arange(vol.N ** 3) * 7 + 3) % 256).astype(np.uint8).reshape((vol.N,) * 3)
    return vol


@pytest.mark.parametrize("fmt", [F32, T16])
@pytest.mark.parametrize("res", [0, 1, 2, 5, 7])
def test_every_upload_path_holds_the_reference(oracle_lib, res, fmt):
    vol = sample_volume(res)
    cell = float(vol.CellSize)
    scale = 0.37 if fmt == T16 else 1.0
    metrics = [(1.0, 0.0), (scale, 0.5 * cell), (1.0, float("inf")), (scale, 2.0 * cell), (1.0, -1.0), (scale, 0.5 * cell)]
    ref = RefCache(R.dense_field(vol.density, fmt), fmt)
    paths = ["float", "float_nomat", "voxels"] + (["texels"] if fmt == T16 else [])
    with v.VHipRenderer() as r:
        for path in paths:
            dense, mat = upload(r, 0, vol, fmt, path)
            assert np.array_equal(dense.view(np.uint32), ref.dense.view(np.uint32)), path
            # a fresh slot starts without tables; then the metric goes to bounded, unbounded (<= 0) and back
            for scale_k, step in metrics:
                set_metric(r, 0, scale_k, step)
                check_slot(r, 0, ref.want(mat, scale_k, step), f"res {res} fmt {fmt} {path} metric ({scale_k}, {step})")
            _abi.check(r._lib.vrt_volume_free(r._ctx, 0), "vrt_volume_free")


@pytest.mark.parametrize("fmt", [F32, T16])
def test_the_benched_256_cubed_shell_holds_the_reference(oracle_lib, fmt):
    vol = scenes.voxelized_torus(8)
    ref = RefCache(R.dense_field(vol.density, fmt), fmt)
    with v.VHipRenderer() as r:
        for path in ("float",) + (("texels",) if fmt == T16 else ()):
            dense, mat = upload(r, 0, vol, fmt, path)
            set_metric(r, 0, vol.density_scale, vol.step_max)
            check_slot(r, 0, ref.want(mat, vol.density_scale, vol.step_max), f"256^3 shell fmt {fmt} {path}")


def test_device_voxelizer_slot_holds_the_reference(oracle_lib):
    """vrt_voxelize_mesh in both formats: the tables derive from the fp32 run's own DENSE (pinned to the CPU converter elsewhere)
    under the shell metric (thr, thr/2), thr = cell * sqrt(3) in fp32; the TEXEL16 run holds that field quantised."""
    from volumetricraytracer_amd import voxelizer as vx

    pos, _, idx = vx.torus_mesh(0.55, 0.22, 64, 32)
    pts, be = vx.importer_space(pos)
    res, extent = 5, float(vx.convert_mesh(pts, idx, be, "torus_5").VolumeExtends)
    N = (1 << res) + 1
    cell = np.float32(np.float32(extent) * np.float32(2.0)) / np.float32(N - 1)
    thr = np.float32(cell * np.sqrt(np.float32(3.0)))
    with v.VHipRenderer() as r:
        fields = {}
        for fmt in (F32, T16):
            _abi.check(r._lib.vrt_set_volume_format(r._ctx, fmt), "vrt_set_volume_format")
            assert r.voxelize_mesh(fmt, pts, idx, res, extent) == 0
            fields[fmt] = read(r, fmt, "dense").view(np.float32).reshape((N,) * 3)
        f32 = fields[F32]
        mat = (f32 <= 0).astype(np.uint8)
        assert mat.sum() > 100
        for fmt in (F32, T16):
            want = RefCache(R.dense_field(f32, fmt), fmt).want(mat, thr, np.float32(0.5) * thr)
            check_slot(r, fmt, want, f"voxelized fmt {fmt}")


def test_every_device_of_a_context_holds_the_reference(oracle_lib):
    vol = scenes.voxelized_torus(6)
    with v.VHipRenderer(devices=(0, 0, 0)) as r:
        for slot, fmt in ((0, T16), (1, F32)):
            dense, mat = upload(r, slot, vol, fmt, "float")
            set_metric(r, slot, vol.density_scale, vol.step_max)
            want = RefCache(dense, fmt).want(mat, vol.density_scale, vol.step_max)
            check_slot(r, slot, want, f"3-device context fmt {fmt}", devices=(0, 1, 2))


@pytest.mark.parametrize("fmt", [F32, T16])
def test_region_edits_hold_the_reference(oracle_lib, fmt):
    """A seeded edit sequence (tests/test_volume_edit_gpu.py) checked against the reference after every edit, not only against a
    full upload."""
    vol = v.torus_volume(5, 100.0, 55.0, 22.0)
    vol.material_id[vol.density <= 0] = 1
    vol.step_max = 0.5 * vol.GetCellSize()
    vol.set_device_format(fmt)
    rng = np.random.default_rng(29 + fmt)
    with v.VHipRenderer() as r:
        upload(r, 0, vol, fmt, "float")
        set_metric(r, 0, vol.density_scale, vol.step_max)
        for i, (o, d, m) in enumerate(edit_sequence(vol, rng)):
            vol.set_region(o, d, m)
            update(r, 0, vol, o, (d.shape[0], d.shape[2], d.shape[1]), records=(i % 4 == 3))
            want = R.device_bytes(R.dense_field(vol.density, fmt), vol.material_id, fmt, vol.density_scale, vol.step_max)
            check_slot(r, 0, want, f"fmt {fmt} edit {i} at {o}")


def non_finite_scene():
    rng = np.random.default_rng(3)
    sc = scenes.config2_sphere(5, 16)
    vol = sc.volumes()[0]
    vol.density = np.array(vol.density, dtype=np.float32, copy=True)
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30, 5e7, -5e7, 400.0]
    for j, (a, b, c) in enumerate(rng.integers(0, vol.N, size=(400, 3))):
        vol.density[a, b, c] = vals[j % len(vals)]
    return sc, vol


def test_non_finite_texel16_densities(oracle_lib):
    """NaN / inf / 1e30 / 5e7 voxels in TEXEL16: vrt_volume_upload and vrt_volume_upload_texels of reference_texels() hold the same
    field (the texel rule), all buffers hold the reference, and frames keep parity with the oracle in the Interp and Cube modes."""
    sc, vol = non_finite_scene()
    vol.set_device_format(T16)
    vol.step_max = 0.5 * vol.GetCellSize()
    field = R.texel16_field(vol.density)
    assert (np.abs(field) == 32767).sum() > 100  # the saturated values are there
    with v.VHipRenderer() as r:
        for slot, path in ((0, "float"), (1, "texels")):
            dense, mat = upload(r, slot, vol, T16, path)
            assert np.array_equal(dense.view(np.uint32), field.view(np.uint32)), path
            set_metric(r, slot, vol.density_scale, vol.step_max)
            check_slot(r, slot, R.device_bytes(field, mat, T16, vol.density_scale, vol.step_max), f"non-finite {path}")
        assert np.array_equal(read(r, 0, "dense"), read(r, 1, "dense"))
        for slot in (0, 1):
            r._lib.vrt_volume_free(r._ctx, slot)
        for mode in (_abi.MODE_INTERP_NOTEX, _abi.MODE_CUBE_NOTEX):
            p = v.default_params(160, 90, vol.GetCellSize(), 255, shadow=True, mode=mode)
            img, t = render(r, sc, p)
            ref, st = OracleScene(sc).render(p, threads=8)
            assert not np.isnan(img).any()
            assert np.abs(img - ref).max() <= TOL, mode
            assert {k: t[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, mode
            assert t["hits"] > 100


def render(r, sc, p):
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)
    img = r.Render()
    return img, r.last_timing()


def test_resolution_9_texel16_holds_the_reference(oracle_lib):
    """N = 513 in TEXEL16 — 2.1 GB of cell records, the largest offsets the kernels address: DENSE exactly; bricks and cell records
    on a seeded sample plus the whole last x-slab; the tables against the oracle's; one PATH_BRICK and one PATH_CELLS frame with
    pixel and counter parity."""
    res = 9
    N = (1 << res) + 1
    g = np.arange(N, dtype=np.float32) * np.float32(200.0 / (N - 1)) - np.float32(100.0)
    vol = v.VVoxelVolume(res, 100.0)
    X, Z, Y = g[:, None, None], g[None, :, None], g[None, None, :]
    vol.density = (np.sqrt(X * X + Y * Y + Z * Z) - np.float32(70.0)).astype(np.float32)
    vol.material_id = (vol.density <= 0).astype(np.uint8)
    vol.Material = v.VMaterial((0.7, 0.8, 0.9, 1.0), 0.8, 0.0)
    vol.step_max = 2.0 * vol.GetCellSize()
    vol.set_device_format(T16)
    sc = v.VScene(Camera=v.look_minus_x_camera(260.0, 30.0), DirectionalLight=v.demo_light(), Objects=[v.VVoxelObject(Volume=vol)],
                  EnvironmentMap=v.procedural_skybox(16))
    nb = R.n_bricks(N)
    rng = np.random.default_rng(9)
    which = np.unique(np.concatenate([rng.integers(0, nb ** 3, 4096), (nb - 1) * nb * nb + np.arange(nb * nb)]))
    with v.VHipRenderer() as r:
        p = v.default_params(128, 72, vol.GetCellSize(), v.march_budget(res), shadow=True, path=_abi.PATH_BRICK)
        img, t = render(r, sc, p)  # uploads the volume (vrt_volume_upload, TEXEL16)
        field = R.texel16_field(vol.density)
        assert_bytes(read(r, 0, "dense"), field.reshape(-1).view(np.uint8), "res 9 dense")
        assert_bytes(read(r, 0, "material"), vol.material_id.reshape(-1), "res 9 material")
        got = read(r, 0, "bricks").view(np.int16).reshape(nb ** 3, 128)
        assert np.array_equal(got[which], R.bricks(field, T16, which)), "res 9 bricks"
        del got
        got = read(r, 0, "cells").view(np.int16).reshape(nb ** 3, 64, 8)
        assert np.array_equal(got[which], R.cells(field, which)), "res 9 cells"
        del got
        o = OracleScene(sc)
        skip, nib, ofield = o.tables(0)
        assert np.array_equal(ofield.view(np.uint32), field.view(np.uint32))
        del ofield, field
        cube, box = o.cube_table(0)
        assert_bytes(read(r, 0, "skip"), R.leap(skip).reshape(-1), "res 9 skip")
        assert_bytes(read(r, 0, "nib"), nib.reshape(-1).view(np.uint8), "res 9 nib")
        assert_bytes(read(r, 0, "cube_skip"), cube.reshape(-1), "res 9 cube_skip")
        assert_bytes(read(r, 0, "active_box"), box.view(np.uint8), "res 9 active box")
        for path in (_abi.PATH_BRICK, _abi.PATH_CELLS):
            p = v.default_params(128, 72, vol.GetCellSize(), v.march_budget(res), shadow=True, path=path)
            frame, stats = (img, t) if path == _abi.PATH_BRICK else render(r, sc, p)
            ref, st = o.render(p, threads=8)
            assert not np.isnan(frame).any()
            assert np.abs(frame - ref).max() <= TOL, path
            assert {k: stats[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, path
            assert stats["hits"] > 500, path
        _abi.check(r._lib.vrt_volume_free(r._ctx, 0), "vrt_volume_free")
