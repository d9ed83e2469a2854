"""Generates tests/golden/ref_held/: what the REFERENCE's own C++ computes, frozen as data.

oracle/_ref/ref_probe (oracle/ref/recipe.py: the reference's Core / Voxel / Scene / Voxelizer sources, compiled unchanged but for
three token rules, linked with our driver oracle/ref/probe.cpp) is run on the cases below and its answers are stored:

  vox_<case>.npz     a mesh and the voxels VVolumeConverter::ConvertMeshInfoToVoxelVolume made of it
  tie_<case>.npz     the same for a box edge placed exactly ON a negative rounding tie (bit-for-bit twins only)
  grid_res<r>.npz    VVoxelVolume's index <-> position rules on ties, negative and out-of-range positions
  octree_<case>.npz  every node of GenerateGPUOctreeStructure for a voxel field (the field is stored too)
  density_<shape>.npz a DensityGenerator shape on a grid
  *.vox              files written by VSerializationManager::SaveToFile
  meta.json          the probe's compiler line and source list, the ExtractResolutionFromName table, the quaternion table of
                     the Eigen stand-in, and what LoadObjectFromFile reads back from each .vox

Nothing here is the reference's program text: inputs we chose, outputs its code wrote while running.
tests/test_ref_held.py regenerates all of it into a temporary directory and compares with the committed files.
Run:  python tests/golden/make_ref_held.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import voxelize_ref as V  # noqa: E402
from test_voxelize_ref import well_cases  # noqa: E402
from volumetricraytracer_amd import voxelizer as vx  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "ref_probe")
BUILD_INFO = os.path.join(ROOT, "oracle", "_ref", "build_info.json")
OUT = os.path.join(HERE, "ref_held")
RECORD = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])
NAMES = ["cube_6", "a_b_4", "plain", "x_9", "x_255", "x_-1", "x_3.7", "x_", "_5", "x_08"]
GRID_RESOLUTIONS = (0, 1, 5, 8)
GRID_EXTENT = 50.0  # cell = 100 / 2^r is a binary fraction: (k + 0.5) * cell - extent is an EXACT tie in fp32
REGION_RESOLUTION = 3


def run(*args) -> str:
    r = subprocess.run([PROBE] + [str(a) for a in args], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"ref_probe {args[0]} failed ({r.returncode}): {r.stderr[-2000:]}")
    return r.stdout


# ---- Voxelizer cases -----------------------------------------------------------------------------------------------------------

def _single(name, resolution, tri, extent=V.EXTENT):
    return V._case(name, resolution, extent, np.asarray(tri, np.float64).reshape(-1, 3, 3))


def region_triangle(k: int) -> V.Case:
    """One seeded triangle inside the volume for region k + 1 of EVTriangleRegion; make_case() asserts from the probe's histogram
    that the converter's classification does put voxels of the triangle's box into that region."""
    rng = np.random.RandomState(300 + k)

    def draw(rng, count):
        c = rng.uniform(-0.3, 0.3, (count, 1, 3)) * V.EXTENT
        return c + rng.uniform(-0.45, 0.45, (count, 3, 3)) * V.EXTENT
    return _single(f"region{k + 1}_res{REGION_RESOLUTION}", REGION_RESOLUTION, V._redrawn(rng, draw, REGION_RESOLUTION, V.EXTENT, 1))


def tetrahedron() -> V.Case:
    """Four faces, resolution 3 (N = 9): the case the recipe was first tried on."""
    p = np.array([[31.0, 29.5, 30.25], [-30.5, -29.0, 31.75], [-29.25, 30.5, -31.0], [30.75, -31.5, -28.5]])
    faces = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
    return _single("tet_res3", 3, [[p[a], p[b], p[c]] for a, b, c in faces])


def far_bounds() -> V.Case:
    """Bounds far larger than the triangles: they stay within +-3 cells of the centre of a 33^3 grid, whose background 2 * extent = 100
    must lie well above every distance the triangles leave in their boxes."""
    rng = np.random.RandomState(41)
    cell = V.grid(5, V.EXTENT)[1]

    def draw(rng, count):
        return rng.uniform(-3.0, 3.0, (count, 3, 3)) * cell
    return _single("far_bounds_res5", 5, V._redrawn(rng, draw, 5, V.EXTENT, 3))


def partly_outside() -> V.Case:
    """Every triangle has a vertex beyond -extent - 2 thr on some axis: GetVoxelizedBoundingBox sees negative coordinates, where
    std::round and floor(x + 0.5) part."""
    rng = np.random.RandomState(42)
    thr = V.grid(4, V.EXTENT)[2]

    def draw(rng, count):
        t = rng.uniform(-0.8, 0.8, (count, 3, 3)) * V.EXTENT
        axis = rng.randint(0, 3, count)
        t[np.arange(count), 0, axis] = -V.EXTENT - rng.uniform(2.0, 6.0, count) * thr
        return t
    return _single("partly_outside_res4", 4, V._redrawn(rng, draw, 4, V.EXTENT, 5))


def torus(resolution: int) -> V.Case:
    """The shell of voxelizer.torus_mesh (48 x 24 quads) in the importer's space, scaled by the first factor (1, 1.001, 1.002 ...) that
    leaves no box edge next to a rounding tie."""
    pos, _, idx = vx.torus_mesh(nu=48, nv=24)
    p, be = vx.importer_space(pos)
    extent = float(np.float32(be.max()) + np.float32(be.max()) * np.float32(0.25))
    for step in range(200):
        q = (p.astype(np.float64) * (1.0 + 1e-3 * step)).astype(np.float32)
        tri = q[idx.reshape(-1, 3)].astype(np.float64)
        if V.boxes(tri, resolution, extent)[2] == 0:
            return V._case(f"torus_res{resolution}", resolution, extent, None, positions=np.ascontiguousarray(q), indices=idx.copy())
    raise AssertionError("torus: no scale without an ambiguous box edge")


TIE_X = -77.900634765625


def tie_case() -> V.Case:
    """NOT one of the Voxelizer cases above, and kept out of the float64 comparison: one triangle wholly outside the volume whose
    largest x is chosen so that the UPPER edge of its box, (max + thr + extent) / cell, is exactly -0.5 in the fp32 sums the converter
    makes (extent 50, N = 9, cell 12.5, thr = fp32(12.5 sqrt 3)).  std::round sends that tie to -1, so the box ends at voxel layer
    x = 0; floor(x + 0.5) would send it to 0 and touch layer x = 1 as well.  It is the one place where the two roundings can be told
    apart after the clip to the grid, and only bit-for-bit twins of the reference (the CPU converter, the device kernel) are held to
    it: make_tie() asserts from the reference's voxels that layer 0 is touched and layer 1 is not, and that the next fp32 value of
    the vertex does touch layer 1."""
    tri = np.array([[TIE_X, -10.0, 5.0], [TIE_X - 20.0, 20.0, -15.0], [TIE_X - 9.5, -25.0, -20.0]], np.float32)
    return V.Case("negative_upper_tie_res3", 3, V.EXTENT, tri, np.arange(3, dtype=np.uint32), 0, True)


def make_tie(work: str) -> dict:
    case = tie_case()
    assert V.boxes(case.triangles(), case.resolution, case.extent)[2] == 1  # the float64 rule calls this edge ambiguous: it is the tie
    out = make_case_arrays(case, work)
    background = np.float32(2.0 * case.extent)
    assert (out["density"][0] < background).any() and (out["density"][1:] == background).all()
    nudged = np.array(case.positions)
    up = np.nextafter(np.float32(TIE_X), np.float32(0.0))
    nudged[:, 0] = [up, up - np.float32(20.0), up - np.float32(9.5)]
    beyond = probe_voxelize(V.Case("nudged", 3, V.EXTENT, nudged, case.indices, 0, True), work)[1]["density"].reshape(9, 9, 9)
    assert (beyond[1] < background).any() and (beyond[2:] == background).all()
    return out


def voxelizer_cases():
    """name -> builder.  The clipped soups and outside-only meshes of tests/test_voxelize_ref.py at resolutions 0, 1, 2, 3 and 5, one
    triangle per region, and the shapes above."""
    out = dict(well_cases(resolutions=(0, 1, 2, 3, 5), others=(1, 5)))
    del out["small_extent_res6"]  # resolution 6: too large a file; the same builder is pinned in test_voxelize_ref.py
    for k in range(7):
        out[f"region{k + 1}_res{REGION_RESOLUTION}"] = lambda k=k: region_triangle(k)
    out["tet_res3"] = tetrahedron
    out["far_bounds_res5"] = far_bounds
    out["partly_outside_res4"] = partly_outside
    out["torus_res5"] = lambda: torus(5)
    return out


def bounds_of(case: V.Case) -> np.float32:
    """The bounds extent b with b + b * 0.25 == extent in fp32 (the converter's own sum)."""
    b = np.float32(case.extent) * np.float32(0.8)
    assert np.float32(b + b * np.float32(0.25)) == np.float32(case.extent), case.name
    return b


def mesh_name(case: V.Case) -> str:
    return f"case_{case.resolution}"


def probe_voxelize(case: V.Case, work: str):
    pos, idx = os.path.join(work, "pos.f32"), os.path.join(work, "idx.u32")
    np.ascontiguousarray(case.positions, np.float32).tofile(pos)
    np.ascontiguousarray(case.indices, np.uint32).tofile(idx)
    b = bounds_of(case)
    out = os.path.join(work, "voxels.rec")
    info = json.loads(run("voxelize", mesh_name(case), pos, idx, repr(float(b)), repr(float(b)), repr(float(b)), out))
    return info, np.fromfile(out, RECORD)


def make_case_arrays(case: V.Case, work: str) -> dict:
    info, rec = probe_voxelize(case, work)
    vol = info["volume"]
    N = vol["size"]
    assert N == (1 << case.resolution) + 1 and rec.size == N ** 3 and vol["resolution"] == case.resolution
    return dict(positions=np.ascontiguousarray(case.positions, np.float32), indices=np.ascontiguousarray(case.indices, np.uint32),
                bounds=np.array([bounds_of(case)] * 3, np.float32), mesh_name=np.array(mesh_name(case)),
                resolution=np.int32(vol["resolution"]), extent=np.float32(vol["extent"]), cell=np.float32(vol["cell"]),
                density=np.ascontiguousarray(rec["density"].reshape(N, N, N)), material=np.ascontiguousarray(rec["material"].reshape(N, N, N)),
                regions=np.array(info["regions"], np.int64))


def make_case(name: str, case: V.Case, work: str) -> dict:
    tri = case.triangles()
    ref = V.reference(tri, case.resolution, case.extent)
    assert ref.ambiguous == 0 and case.skipped == 0 and case.well, name
    out = make_case_arrays(case, work)
    regions, density, N = out["regions"], out["density"], out["density"].shape[0]
    if name.startswith("region"):
        k = int(name[6]) - 1
        assert regions[k] > 0, (name, regions)
    if name.startswith("far_bounds"):
        assert np.float32(2.0 * case.extent) > 10.0 * density[ref.covered].max() and (~ref.covered).sum() > 0.5 * N ** 3
    if name.startswith("partly_outside"):
        cell, thr = V.grid(case.resolution, case.extent)[1:]
        assert (((tri.min(axis=1) - thr + case.extent) / cell) < -1.0).any(axis=1).all()
    return out


# ---- grid ----------------------------------------------------------------------------------------------------------------------

def grid_inputs(resolution: int):
    """Positions: exact ties (k + 0.5 cells from the origin corner), 1e-3 cells either side, on voxels, negative (k = -2, -1),
    at +-extent and beyond; each value on one axis at a time (the others at 0.3 cells) and on all three.  Indices: the corners, the
    last valid ones, one beyond each way."""
    N, cell, _ = V.grid(resolution, GRID_EXTENT)
    ks = sorted({-2, -1, 0, 1, (N - 1) // 2, N - 2, N - 1, N})
    rel = []
    for k in ks:
        rel += [k + 0.5, k + 0.5 - 1e-3, k + 0.5 + 1e-3, float(k), k + 0.25]
    values = [np.float32(np.float32(r) * np.float32(cell)) - np.float32(GRID_EXTENT) for r in rel]
    values += [np.float32(GRID_EXTENT), np.float32(-GRID_EXTENT), np.float32(1.3 * GRID_EXTENT), np.float32(-1.3 * GRID_EXTENT),
               np.float32(4.0 * GRID_EXTENT), np.float32(-4.0 * GRID_EXTENT)]
    base = np.float32(np.float32(0.3) * np.float32(cell)) - np.float32(GRID_EXTENT)
    pos = []
    for v in values:
        pos += [[v, base, base], [base, v, base], [base, base, v], [v, v, v]]
    idx = [[0, 0, 0], [N - 1, N - 1, N - 1], [N - 1, 0, 0], [0, N - 1, 0], [0, 0, N - 1], [1 % N, 2 % N, 3 % N], [N, 0, 0], [0, N, 0], [0, 0, N],
           [-1, 0, 0], [0, -1, 0], [0, 0, -1], [N // 2, N // 3, N // 4]]
    return np.array(pos, np.float32), np.array(idx, np.int32)


def make_grid(resolution: int, work: str) -> dict:
    pos, idx = grid_inputs(resolution)
    pf, jf, out = os.path.join(work, "gp.f32"), os.path.join(work, "gi.i32"), os.path.join(work, "grid")
    pos.tofile(pf)
    idx.tofile(jf)
    info = json.loads(run("grid", resolution, repr(GRID_EXTENT), pf, jf, out))
    return dict(resolution=np.int32(resolution), extent=np.float32(GRID_EXTENT), size=np.int32(info["size"]), voxel_count=np.int64(info["voxel_count"]),
                cell=np.float32(info["cell"]), positions=pos, indices=idx,
                voxel_index=np.fromfile(out + ".voxel_index", np.int32).reshape(-1, 3), cell_index=np.fromfile(out + ".cell_index", np.int32).reshape(-1, 3),
                index_position=np.fromfile(out + ".position", np.float32).reshape(-1, 3), valid=np.fromfile(out + ".valid", np.uint8),
                flat=np.fromfile(out + ".flat", np.int64))


# ---- octree --------------------------------------------------------------------------------------------------------------------

def _field(resolution, fn):
    N = (1 << resolution) + 1
    g = np.linspace(-1.0, 1.0, N)
    X, Z, Y = np.meshgrid(g, g, g, indexing="ij")  # arrays are [x, z, y]: Index3DTo1D = x*N*N + z*N + y
    return np.ascontiguousarray(fn(X, Y, Z), np.float32)


def octree_fields(work: str):
    """name -> (resolution, density [x, z, y]); the material is (density <= 0), as both of the reference's producers write it."""
    one_corner = np.full((9, 9, 9), 3.0, np.float32)
    one_corner[8, 8, 8] = -1.0
    zero_sample = _field(2, lambda X, Y, Z: 0.4 + 0.0 * X)
    zero_sample[2, 1, 3] = 0.0
    res1 = _field(1, lambda X, Y, Z: X + 0.3)
    res0_flat = np.full((2, 2, 2), 1.0, np.float32)
    res0_cut = _field(0, lambda X, Y, Z: Z + 0.5)
    torus6 = probe_voxelize(torus(6), work)[1]["density"].reshape(65, 65, 65)
    return {
        "all_positive_res3": (3, np.full((9, 9, 9), 2.5, np.float32)),
        "all_negative_res3": (3, np.full((9, 9, 9), -2.5, np.float32)),
        "one_corner_res3": (3, one_corner),
        "sphere_res5": (5, _field(5, lambda X, Y, Z: np.sqrt(X * X + Y * Y + Z * Z) - 0.6)),
        "torus_res6": (6, np.ascontiguousarray(torus6)),
        "res0_flat": (0, res0_flat),
        "res0_cut": (0, res0_cut),
        "res1_cut": (1, res1),
        "zero_on_sample_res2": (2, zero_sample),
    }


def make_octree(resolution: int, density: np.ndarray, work: str) -> dict:
    N = (1 << resolution) + 1
    rec = np.zeros(N ** 3, RECORD)
    rec["density"] = density.reshape(-1)
    rec["material"] = (density.reshape(-1) <= 0).astype(np.uint8)
    vf, out = os.path.join(work, "oct.rec"), os.path.join(work, "oct.nodes")
    rec.tofile(vf)
    info = json.loads(run("octree", resolution, vf, out))
    nodes = np.fromfile(out, np.int32).reshape(-1, 28)
    assert len(nodes) == info["nodes"]
    # the field itself as sign bits + the few values that matter to nobody: signs are all the octree reads
    return dict(resolution=np.int32(resolution), axis=np.int32(info["axis"]), is_leaf=nodes[:, 0].astype(np.uint8),
                cell_index=nodes[:, 1:4].astype(np.int16), children=nodes[:, 4:].reshape(-1, 8, 3).astype(np.int16),
                sign=np.sign(density).astype(np.int8))


# ---- density -------------------------------------------------------------------------------------------------------------------

DENSITY_SHAPES = {
    # name: (probe arguments after "density RES EXTENT OUT", ...) — resolution 4, extent 100
    "sphere": ["sphere", 40.0, 5.0, -7.0, 3.0, 0.0, 0.0, 0.0, 1.0],
    "box": ["box", 30.0, 45.0, 20.0, 4.0, 2.0, -6.0, 0.18257418, 0.36514837, 0.54772256, 0.73029674],
    "cylinder": ["cylinder", 25.0, 50.0, -3.0, 8.0, 1.0, 0.0, 0.38268343, 0.0, 0.92387953],
}


def make_density(shape: str, work: str) -> dict:
    out = os.path.join(work, "density.f32")
    args = DENSITY_SHAPES[shape]
    info = json.loads(run("density", 4, repr(100.0), out, args[0], *[repr(float(a)) for a in args[1:]]))
    N = info["size"]
    return dict(resolution=np.int32(4), extent=np.float32(100.0), params=np.array(args[1:], np.float32),
                density=np.fromfile(out, np.float32).reshape(N, N, N))


# ---- .vox ----------------------------------------------------------------------------------------------------------------------

VOX_VOLUMES = {
    # name: (colour, roughness, metallic, texture scale, albedo, normal, rm)
    "volume_default": ((0.8, 0.8, 0.8, 1.0), 0.8, 0.0, (100.0, 100.0), "", "", ""),
    "volume_textured": ((0.25, 0.5, 0.75, 1.0), 0.35, 0.6, (25.0, 40.0), "tex/albedo.png", "tex/normal.png", "tex/rm.png"),
}


def vox_field():
    d = _field(2, lambda X, Y, Z: np.sqrt(X * X + Y * Y + Z * Z) * 50.0 - 31.0)
    rec = np.zeros(d.size, RECORD)
    rec["density"] = d.reshape(-1)
    rec["material"] = (d.reshape(-1) <= 0).astype(np.uint8)
    return rec


def scene_manifest(work: str) -> str:
    """Two meshes (told apart by rising roughness, which the probe uses to fix the file's volume order: V_0 is the last mesh), one object of each, the
    directional light, a point light, a spot light, a camera (which the format does not store: the read-back shows it)."""
    lines = []
    for k, (case, rough) in enumerate(((tetrahedron(), 0.3), (region_triangle(0), 0.6))):
        pos, idx = os.path.join(work, f"m{k}.f32"), os.path.join(work, f"m{k}.u32")
        np.ascontiguousarray(case.positions, np.float32).tofile(pos)
        np.ascontiguousarray(case.indices, np.uint32).tofile(idx)
        b = float(bounds_of(case))
        lines.append(f"mesh mesh{k}_2 {pos} {idx} {b!r} {b!r} {b!r} {0.2 + 0.3 * k} 0.5 {0.9 - 0.3 * k} 1 {rough} {0.1 * k}")
    lines.append("object mesh0_2 10 -20 30 1 2 0.5 0 0 0.38268343 0.92387953")
    lines.append("object mesh1_2 -40 15 5 1.5 1.5 1.5 0.5 0.5 0.5 0.5")
    lines.append("light directional 0 0 0 0.27059805 0.27059805 0.65328148 0.65328148 1 0.95 0.9 1 6 0 0 0 0")
    lines.append("light point 5 60 70 0 0 0 1 0.2 0.4 1 1 40 0.25 0.01 0 0")
    lines.append("light spot -70 -60 90 0 0.70710678 0 0.70710678 1 0.5 0.25 1 30 0.125 0.02 15 50")
    lines.append("camera 250 0 40 0 0 1 0 55")
    path = os.path.join(work, "scene.manifest")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def read_back(kind: str, path: str, work: str) -> dict:
    prefix = os.path.join(work, "rb")
    info = json.loads(run("vox-read", kind, path, prefix))
    for k, vol in enumerate(info["volumes"]):
        rec = np.fromfile(prefix + f".v{k}", RECORD)
        vol["density_bits"] = [int(x) for x in rec["density"].view(np.uint32)]
        vol["materials"] = [int(x) for x in rec["material"]]
        for key in ("albedo", "normal", "rm"):  # the reference resolves relative paths against the file's folder: keep what follows it
            folder = os.path.dirname(path) + os.sep
            if vol["material"][key].startswith(folder):
                vol["material"][key] = "<folder>/" + vol["material"][key][len(folder):]
    return info


def make_vox(out_dir: str, work: str) -> dict:
    """Writes the .vox files into out_dir; returns what the reference reads back from each."""
    rec_path = os.path.join(work, "vox.rec")
    vox_field().tofile(rec_path)
    back = {}
    for name, (col, rough, metal, ts, a, n, rm) in VOX_VOLUMES.items():
        path = os.path.join(out_dir, name + ".vox")
        run("vox-write-volume", 2, repr(100.0), rec_path, *col, rough, metal, *ts, a, n, rm, path)
        back[name] = read_back("volume", path, work)
    path = os.path.join(out_dir, "scene.vox")
    run("vox-write-scene", scene_manifest(work), path)
    back["scene"] = read_back("scene", path, work)
    return back


# ---- the Eigen stand-in's own table --------------------------------------------------------------------------------------------

def quat_inputs() -> np.ndarray:
    """12 seeded rows: q1 and q2 (xyzw; the first 8 rows unit, the last 4 of length 0.5 .. 2), v, a, b."""
    rng = np.random.RandomState(2024)
    q = rng.normal(size=(12, 2, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    q[8:] *= rng.uniform(0.5, 2.0, (4, 2, 1))
    rows = np.concatenate([q.reshape(12, 8), rng.uniform(-100, 100, (12, 3)), rng.normal(size=(12, 3)) * 10, rng.normal(size=(12, 3))], axis=1)
    return np.ascontiguousarray(rows, np.float32)


def make_quat(work: str) -> np.ndarray:
    fin, fout = os.path.join(work, "q.in"), os.path.join(work, "q.out")
    quat_inputs().tofile(fin)
    run("quat", fin, fout)
    return np.fromfile(fout, np.float32).reshape(12, 15)


# ---- everything ----------------------------------------------------------------------------------------------------------------

def generate(out_dir: str) -> None:
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as work:
        for name, build in voxelizer_cases().items():
            np.savez_compressed(os.path.join(out_dir, f"vox_{name}.npz"), **make_case(name, build(), work))
        np.savez_compressed(os.path.join(out_dir, "tie_negative_upper_tie_res3.npz"), **make_tie(work))
        for r in GRID_RESOLUTIONS:
            np.savez_compressed(os.path.join(out_dir, f"grid_res{r}.npz"), **make_grid(r, work))
        for name, (r, density) in octree_fields(work).items():
            np.savez_compressed(os.path.join(out_dir, f"octree_{name}.npz"), **make_octree(r, density, work))
        for shape in DENSITY_SHAPES:
            np.savez_compressed(os.path.join(out_dir, f"density_{shape}.npz"), **make_density(shape, work))
        back = make_vox(out_dir, work)
        with open(BUILD_INFO) as f:
            info = json.load(f)
        meta = {"compiler_line": info["compiler_line"], "reference_files": info["files"], "token_rules": info["rules"],
                "names": json.loads(run("names", *NAMES)), "quat": [[int(b) for b in row.view(np.uint32)] for row in make_quat(work)],
                "vox_read_back": back}
        with open(os.path.join(out_dir, "meta.json"), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    generate(OUT)
    sizes = sorted(((os.path.getsize(os.path.join(OUT, n)), n) for n in os.listdir(OUT)), reverse=True)
    print(f"{len(sizes)} files, {sum(s for s, _ in sizes)} bytes; largest: {sizes[:3]}")
