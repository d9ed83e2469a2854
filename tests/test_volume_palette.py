"""Per-voxel materials without a GPU: the C-ABI, header, Python and adaptor surface of vrt_volume_set_palette / _get_palette; the unit
cases of the rule that gives a hit its entry (tests/palette_ref.py, restating include/vrt.h); and the painted sphere of the GPU tests
under the CPU oracle's own hits: the share of hit pixels too near a decision boundary to be compared bit for bit stays below the cap,
and both painted ids show."""
import ctypes as C
import os

import numpy as np

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from oracle.binding import OracleScene

import brush_ref
import palette_ref as pr
from volume_ref import F32, TEXEL16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_the_library_exports_the_palette_calls_and_refuses_null():
    lib = _abi.load()
    n = C.c_int(7)
    assert lib.vrt_volume_set_palette(None, 0, 0, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_get_palette(None, 0, 0, None, C.byref(n)) == _abi.VRT_ERR_INVALID
    assert _abi.FORM_PALETTE == 32 and _abi.VRT_MAX_PALETTE == 256
    assert hasattr(v.VHipRenderer, "set_palette") and hasattr(v.VHipRenderer, "get_palette")


def test_header_python_and_adaptor_name_the_call():
    header = open(os.path.join(ROOT, "include", "vrt.h")).read()
    assert "int vrt_volume_set_palette(vrt_ctx* ctx, int slot, int n, const vrt_material* entries_or_null);" in header
    assert "int vrt_volume_get_palette(vrt_ctx* ctx, int slot, int capacity, vrt_material* entries_or_null, int* n_out);" in header
    assert "#define VRT_MAX_PALETTE 256" in header and "#define VRT_FORM_PALETTE 32" in header
    assert " *   vrt_volume_set_palette," in header[:header.index("#ifndef VRT_H")]  # the entry-point list
    adaptor = open(os.path.join(ROOT, "volumetricraytracer_amd", "csrc", "host", "HipRenderer.h")).read()
    assert "bool SetPalette(const Scene::VVoxelObject& object, const std::vector<VMaterial>& entries);" in adaptor
    assert "bool ClearPalette(const Scene::VVoxelObject& object);" in adaptor


# ---- the rule's unit cases: a 3^3 grid of cells of 1.0 (N = 3, extent 1), the point in cell (0, 0, 0) -----------------------------------
def _grid(outside=1.0):
    d = np.full((3, 3, 3), outside, f32)   # [x, z, y]
    m = np.zeros((3, 3, 3), np.uint8)
    return d, m


def _at(fx, fy, fz):
    return np.array([[fx - 1.0, fy - 1.0, fz - 1.0]])  # p = g * cell - extent


def test_a_tie_goes_to_the_lowest_corner():
    d, m = _grid()
    d[0, 0, 0] = d[1, 0, 0] = -1.0           # corners j = 0 (0,0,0) and j = 1 (1,0,0)
    m[0, 0, 0], m[1, 0, 0] = 5, 6
    ids, dist = pr.entry_ids(d, m, 1.0, _at(0.5, 0.25, 0.25))
    assert ids[0] == 5 and dist[0] == 0.0    # on the bisector itself
    assert pr.entry_ids(d, m, 1.0, _at(0.75, 0.25, 0.25))[0][0] == 6
    d[0, 0, 0] = 1.0                         # j = 0 outside now: j = 1 against j = 2 (0,1,0)
    d[0, 0, 1] = -1.0
    m[0, 0, 1] = 7
    assert pr.entry_ids(d, m, 1.0, _at(0.5, 0.5, 0.25))[0][0] == 6


def test_without_an_inside_corner_the_nearest_sample_decides():
    d, m = _grid()
    m[1, 0, 1] = 9                           # sample (x, y, z) = (1, 1, 0), an outside one
    ids, dist = pr.entry_ids(d, m, 1.0, _at(0.75, 0.5 + 0.125, 0.25))
    assert ids[0] == 9 and abs(dist[0] - 0.125) < 1e-6
    assert pr.entry_ids(d, m, 1.0, _at(0.25, 0.25, 0.25))[0][0] == 0


def test_nan_is_never_inside_and_minus_zero_is():
    d, m = _grid()
    d[0, 0, 0] = np.nan
    d[1, 1, 1] = -0.0
    m[0, 0, 0], m[1, 1, 1] = 3, 4
    assert pr.entry_ids(d, m, 1.0, _at(0.125, 0.125, 0.125))[0][0] == 4  # the far corner, the only INSIDE one
    d[1, 1, 1] = 0.0
    assert pr.entry_ids(d, m, 1.0, _at(0.125, 0.125, 0.125))[0][0] == 4  # +0 <= 0 too
    d[1, 1, 1] = np.nan
    assert pr.entry_ids(d, m, 1.0, _at(0.125, 0.125, 0.125))[0][0] == 3  # none INSIDE: the nearest sample, NaN or not


def test_a_texel16_slot_decides_by_the_stored_fields_sign():
    stored = np.array([-0.0, 0.0, 3.0, -3.0, -32767.0], f32)  # the integer field +-q as the device keeps it
    decoded = brush_ref.decode(stored, TEXEL16)
    assert np.array_equal(decoded <= 0, [True, True, False, True, True]) and np.signbit(decoded[0])
    d, m = _grid(outside=brush_ref.decode(f32(30.0), TEXEL16))
    d[0, 0, 0] = decoded[0]                  # a small negative density quantises to -0: still INSIDE
    m[0, 0, 0] = 8
    assert pr.entry_ids(d, m, 1.0, _at(0.75, 0.75, 0.75))[0][0] == 8
    assert np.array_equal(brush_ref.decode(stored, F32), stored)


def test_the_clamped_cell_at_the_grids_far_faces():
    d, m = _grid()
    d[2, 2, 2] = -1.0
    m[2, 2, 2] = 2
    ids, _ = pr.entry_ids(d, m, 1.0, np.array([[1.0, 1.0, 1.0], [1.5, 0.9, 0.9]]))  # on the far corner; beyond the grid
    assert list(ids) == [2, 2]


# ---- the painted sphere under the oracle -------------------------------------------------------------------------------------------
def test_the_test_scenes_exclusion_share_and_both_ids(oracle_lib):
    vol = pr.sphere_volume()
    stored, material = vol.density.copy(), vol.material_id.copy()
    assert set(np.unique(material)) == {0, 1} and np.array_equal(material == 1, stored <= 0)
    res = brush_ref.apply(stored, material, F32, [pr.paint_record()], pr.EXTENT, 1.0)
    assert res["written"] > 0 and np.array_equal(stored, vol.density)
    x = np.arange(vol.N)[:, None, None]
    assert np.array_equal(material == 2, (stored <= 0) & (x > pr.PAINT_X)) and np.array_equal(material == 1, (stored <= 0) & (x < pr.PAINT_X))
    sc = pr.painted_sphere_scene(vol)
    p = pr.scene_params(sc)
    osc = OracleScene(sc)
    o, d = osc.camera_rays(pr.WIDTH, pr.HEIGHT, pr.all_pixels())
    hit, t, _ = osc.trace_batch(p, o, d, threads=8)
    obj = sc.Objects[0]
    pts = pr.object_points(obj.Position, obj.Rotation, obj.Scale, o[hit], d[hit], t[hit])
    ids, dist = pr.entry_ids(stored, material, pr.EXTENT, pts)
    n = int(hit.sum())
    excluded = int((dist < pr.MARGIN_CELLS).sum())
    shares = {k: float((ids == k).sum()) / n for k in (0, 1, 2)}
    print(f"hit pixels {n}, excluded {excluded} ({100.0 * excluded / n:.2f} %), id shares {shares}")
    assert n > 500  # the sphere fills a good part of the 96 x 54 frame
    assert excluded < pr.EXCLUDED_CAP * n
    assert shares[1] >= 0.10 and shares[2] >= 0.10
    assert shares[0] < 0.02  # id 0 only where the ray stopped, a threshold short of the surface, in a cell without an INSIDE corner
