"""The cases that the tests of the volume calls at the smallest and the largest resolutions share (tests/test_volume_ops_extremes.py
on the host passes, tests/test_volume_ops_extremes_gpu.py on the device): fields, case tables and the builders of the large inputs.
Everything is built once and never written to afterwards."""
from __future__ import annotations

import functools

import numpy as np

import brush_ref as B
import fill_ref as F
import redistance_ref as RR
import stamp_cases as K
import stamp_ref as S
import volume_ref as R
import volumetricraytracer_amd as v

SMALL = (2, 3, 5)  # resolutions 0, 1, 2: one brick, one 8^3 tile, one partial run of cells
FORMATS = (R.F32, R.TEXEL16)
EXTENT, SCALE = 6.0, 0.5
CAP = 1 << 24  # lanes of a capped grid-stride launch: 65 536 workgroups of 256


def resolution(N: int) -> int:
    return int(N - 1).bit_length() - 1


def read_only(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def volume(N: int, fmt: int, table: bool, extent: float = EXTENT, scale: float = SCALE) -> v.VVoxelVolume:
    """An empty volume of N^3 samples carrying the metric: with (step_max > 0) or without the empty-space tables on the device."""
    vol = v.VVoxelVolume(resolution(N), extent)
    assert vol.N == N
    vol.density_scale = scale
    vol.step_max = 1.5 * vol.GetCellSize() if table else 0.0
    return vol.set_device_format(fmt)


# ---- resolutions 0, 1, 2 -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_field(N: int) -> np.ndarray:
    """Seeded normal densities of about a cell's size (a cell is 2 * EXTENT / (N - 1) / SCALE density units) with both signs at every N,
    and — where the grid has room — a NaN, a +0 and a -0 sample, each next to samples of both signs."""
    rng = np.random.default_rng(40 + N)
    d = rng.standard_normal((N, N, N)).astype(np.float32)
    d[0, 0, 0], d[N - 1, N - 1, N - 1] = np.float32(-0.8), np.float32(0.9)  # both classes whatever the seed gives
    if N >= 3:
        d[1, 1, 1], d[0, 2, 1], d[2, 0, 1] = np.float32(np.nan), np.float32(0.0), np.float32(-0.0)
    return read_only(d)


@functools.lru_cache(maxsize=None)
def small_field(N: int, fmt: int):
    """(stored, material): random_field(N) as a slot of the format stores it — in TEXEL16 by the texel rule: NaN and +-0 become +0, a
    negative below one quantum -0 — and ids that differ from sample to sample."""
    return read_only(R.dense_field(random_field(N), fmt), F.hand_made_material(np.array(random_field(N))))


def unit_of(N: int, extent: float = EXTENT, scale: float = SCALE) -> np.float32:
    return B.units(N, extent, scale)[1]


def fill_fields(N: int) -> dict:
    """name -> (density, filled, lo, hi): solid (-1) with the samples that lie on no face at 0.5, and the same with one face sample
    next to them (x = 0) opened.  N = 2 has no such sample: nothing can be enclosed."""
    sealed = np.full((N, N, N), -1.0, np.float32)
    sealed[1:N - 1, 1:N - 1, 1:N - 1] = np.float32(0.5)
    opened = sealed.copy()
    opened[0, N // 2, N // 2] = np.float32(0.5)
    inner = max(N - 2, 0) ** 3
    return {"sealed": (sealed, inner, (1, 1, 1) if inner else None, (N - 2,) * 3 if inner else None), "opened": (opened, 0, None, None)}


REDISTANCE_BANDS = (1, 7, 8, 15)  # both ring counts of a tiled implementation; every one but 1 is wider than these grids
REDISTANCE_FROMS = (RR.BOTH, RR.OUTSIDE, RR.INSIDE)


def redistance_boxes(N: int) -> dict:
    return {"whole grid": (None, None), "one sample": ((N // 2, N - 1, 0), (N // 2, N - 1, 0))}


def redistance_runs(N: int):
    return [(band, from_, box) for band in REDISTANCE_BANDS for from_ in REDISTANCE_FROMS for box in redistance_boxes(N)]


MESH_ISOS = (0.0, 0.3)


def mesh_boxes(N: int) -> dict:
    """The whole grid and, at N = 5, 2 x 5 x 3 samples (x, y, z): one cell along x, a whole row along y, two cells along z."""
    out = {"whole grid": (None, None)}
    if N == 5:
        out["2 x 5 x 3"] = ((1, 0, 1), (2, 4, 3))
    return out


STAMP_SIZES = ((2, 2), (3, 5), (5, 2), (5, 3), (17, 2))  # (Nd, Ns): a source of Ns = 2 has Ns - 2 = 0 as its only cell
STAMP_PLACEMENTS = ("identity", "axis turn 0", "oblique 1", "u lands on Ns - 1")


def stamp_cases(Nd: int, Ns: int):
    """(what, source field, destination field, record) as stamp_cases.sweep yields them: the four placements with the three ops, the
    source's material ids, blend cycling.  The fields are stamp_cases' random normal ones with their NaN, inf and +-0 samples — but
    for a source of Ns = 2, whose single cell would hand its one NaN to every sample of the destination: that one is plain normal."""
    src = "normal" if Ns == 2 else "hand"
    n = 0
    for name, matrix, scale in K.placements(Nd, Ns):
        if not any(name.startswith(p) for p in STAMP_PLACEMENTS):
            continue
        for op in K.OPS:
            blend = K.BLENDS[n % 2]
            yield f"{name}, op {op}, blend {blend}", src, "hand", K.record(op, matrix, scale, blend, S.SOURCE, 0.0)
            n += 1


# ---- 257^3 and 513^3 -----------------------------------------------------------------------------------------------------------------

def split_by_cap(mask: np.ndarray):
    """(samples of the mask below CAP, at or above it) in linear order."""
    flat = mask.reshape(-1)
    return int(flat[:CAP].sum()), int(flat[CAP:].sum())


@functools.lru_cache(maxsize=None)
def torus_257():
    """(density, material) of an analytic torus on 257^3, solid ids 1."""
    vol = v.torus_volume(8, 100.0, 55.0, 22.0)
    d = np.array(vol.density, np.float32)
    return read_only(d, (d <= 0).astype(np.uint8))


def brush_calls_257():
    """Two calls whose records' union box is the whole 257^3 grid.  The first: a hard ADD sphere of 100 cells about the centre whose
    reach of 110 stops short of the grid's corners (128 * sqrt(3) = 221.7 > 210), a blended ADD ball on the face x = 256 and a blended
    SUBTRACT bite out of it, all beyond lane 2^24.  The second, one record: a hard SUBTRACT ball at x = 250 whose reach spans the grid
    but which writes only where -v exceeds the field."""
    first = [v.sphere_brush(B.ADD, (128.0, 128.0, 128.0), 100.0, 0.0, 110.0, 2),
             v.sphere_brush(B.ADD, (255.2, 128.3, 127.6), 6.0, 2.0, 3.0, 5),
             v.sphere_brush(B.SUBTRACT, (254.5, 124.0, 130.0), 4.0, 1.0, 2.0, 0)]
    second = [v.sphere_brush(B.SUBTRACT, (250.0, 128.0, 128.0), 12.0, 0.0, 450.0, 0)]
    return first, second


def cavity_field(N: int, x0: int, x1: int, solid: float = -1.0, hollow: float = 0.5) -> tuple:
    """(density, cavities, channel): solid (-1) with sealed cavities (0.5) across x = x0 .. x1, in x = x1 alone and near the origin,
    and a channel (0.5) three samples long that opens on the face x = N - 1 and so must stay unfilled.  Boxes are (lo, hi) xyz
    inclusive."""
    d = np.full((N, N, N), solid, np.float32)
    cavities = [((x0, 100, 100), (x1, 102, 102)), ((x1, 50, 60), (x1, 52, 62)), ((2, 2, 2), (4, 4, 4))]
    channel = ((N - 3, 200, 200), (N - 1, 200, 200))
    for lo, hi in cavities + [channel]:
        F._box(d, lo, hi, hollow)
    return d, cavities, channel


def sphere_in_constant(N: int, centre, radius: float, unit: float, far: float = 30.0, margin: int = 12):
    """(density, material): far everywhere but in the block of samples within radius + margin cells of the centre on each axis, which
    holds the signed distance to the sphere (density units) and ids that differ from sample to sample."""
    d = np.full((N, N, N), far, np.float32)
    m = np.zeros((N, N, N), np.uint8)
    lo = [max(0, int(c - radius - margin)) for c in centre]
    hi = [min(N - 1, int(c + radius + margin)) for c in centre]
    x = np.arange(lo[0], hi[0] + 1, dtype=np.float64)[:, None, None]
    z = np.arange(lo[2], hi[2] + 1, dtype=np.float64)[None, :, None]
    y = np.arange(lo[1], hi[1] + 1, dtype=np.float64)[None, None, :]
    block = ((np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius) * unit).astype(np.float32)
    assert float(block[0].min()) > 0 and float(block[:, 0].min()) > 0 and float(block[:, :, 0].min()) > 0  # no surface on the block's faces
    at = (slice(lo[0], hi[0] + 1), slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1))
    d[at] = block
    m[at] = F.hand_made_material(block)
    return d, m


# ---- frames around an edit -----------------------------------------------------------------------------------------------------------

EDIT_OPS = ("stamp", "fill", "redistance", "smooth", "warp", "components")
ANALYTIC_OPS = ("stamp", "smooth", "warp", "components")  # on config3_torus(6); the others on the Voxelizer's shell of it


def stamp_source():
    """The 17^3 sphere of stamp_cases, as a volume of its own."""
    return K.volume("sphere", 17, "src")


def frame_stamp(vol) -> object:
    """A SUBTRACT of the 17^3 sphere at 0.6 of its size out of the side of config3_torus(6) that faces the camera (the ring runs 17.6
    cells out with a tube of 7 cells)."""
    c = (vol.N - 1) / 2.0
    return v.stamp_from_placement(17, (c + 18.0, c, c + 8.0), K.quat((1, 1, 0), 30.0), 0.6, op=S.SUBTRACT, material=0)


def frame_smooth(vol) -> object:
    """A dab of 6 cells on the side of config3_torus(6) that faces the camera: the tube's outer equator lies 24.6 cells out along +x."""
    c = (vol.N - 1) / 2.0
    return v.smooth_record(B.SPHERE, (c + 22.0, c + 0.4, c + 4.0), (0.0, 0.0, 0.0), 6.0, strength=1.0, iterations=8, falloff=2.0)


def frame_warp(vol) -> object:
    """A ball of 9 cells about the tube's outer equator grabbed by 4.5 cells outwards, towards the camera: the surface ends 29 cells out,
    in a brick beyond the active box's last one (the box ends with the brick of cell 32 + 24.6 + 0.5: brick 14 of 16)."""
    c = (vol.N - 1) / 2.0
    pull = v.warp_from_motion((0.0, 0.0, 0.0), translation=(4.5, 0.0, 1.0))[0]
    return v.warp_record(B.SPHERE, (c + 22.0, c, c + 2.0), (0.0, 0.0, 0.0), 9.0, pull=pull, falloff=4.0, material=-2)


def frame_island(vol) -> object:
    """A ball of 3 cells above the torus' hole on the camera's side, 15.9 cells from the ring's centre line: an island of its own."""
    c = (vol.N - 1) / 2.0
    return v.sphere_brush(B.ADD, (c + 10.0, c, c + 14.0), 3.0, 0.0, 2.0, 1)


def frame_components(vol) -> object:
    """Every component of fewer than 1000 samples goes — the island has about 113, the torus 13 000 — and leaves a gap of half a cell."""
    from volumetricraytracer_amd import _abi
    return _abi.components_record(_abi.COMPONENTS_REMOVE_SMALL, gap=0.5 * float(B.units(vol.N, vol.VolumeExtends, vol.density_scale)[1]),
                                  material=0, min_samples=1000)


def edit_scene(op: str):
    """(scene, its volume) for the frames around `op`, F32 so that the oracle marches the host mirror: the analytic torus for the stamp,
    the smooth, the warp and the components call, the Voxelizer's shell of it for the fill and the redistance."""
    from volumetricraytracer_amd import workloads as scenes
    if op in ANALYTIC_OPS:
        sc = scenes.config3_torus(6, 16)
        vol = sc.volumes()[0]
        vol.step_max = 0.5 * vol.GetCellSize()
    else:
        sc = scenes.config3_voxelized(5, 16)
        vol = sc.volumes()[0]
    vol.density, vol.material_id = np.array(vol.density, np.float32), np.array(vol.material_id, np.uint8)
    return sc, vol


def host_edit(op: str, vol, prepare_only: bool = False):
    """The host pass of what device_edit does, on the host volume in place: the fill that precedes the redistance and the island that
    the components call removes (prepare; the brush by its numpy rule, tests/brush_ref.py), then the op itself."""
    from volumetricraytracer_amd import voxelizer as vx
    if op == "redistance":
        vx.fill_enclosed_host(vol, 1.0, 1)
    if op == "components":
        got = B.apply(vol.density, vol.material_id, R.F32, [frame_island(vol)], vol.VolumeExtends, vol.density_scale)
        assert got["written"] > 50, got
    if prepare_only:
        return
    if op == "stamp":
        vx.stamp_host(vol, stamp_source(), frame_stamp(vol))
    elif op == "fill":
        vx.fill_enclosed_host(vol, 1.0, 1)
    elif op == "smooth":
        assert vx.smooth_host(vol, frame_smooth(vol))["written"] > 100
    elif op == "warp":
        assert vx.warp_host(vol, frame_warp(vol))["written"] > 100
    elif op == "components":
        got = vx.components_host(vol, frame_components(vol))
        assert got["removed"] == 1 and got["written"] > 50, got
    else:
        vx.redistance_host(vol, 3, RR.OUTSIDE)
