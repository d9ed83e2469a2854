"""Plain-numpy reference of vrt_volume_fill_enclosed, written from the contract in include/vrt.h rather than from either C++ build:
whole [x, z, y] arrays, a dilation of the six faces' seeds under the passable mask until nothing changes.  The arithmetic is
np.float32: one add, one negation.

The state is what the device stores, as in brush_ref: `stored` is the DENSE buffer (F32: the densities; TEXEL16: the integer field
+-q as float32) and `material` the material ids.  fill() leaves both alone and returns edited copies.

hand_made_fields() builds the 33^3 fields of tests/test_volume_fill*.py: the smallest shapes at which a flood can go wrong."""
from __future__ import annotations

import numpy as np

from volume_ref import F32, TEXEL16, texel16_field

f32 = np.float32


def decode(stored: np.ndarray, fmt: int) -> np.ndarray:
    """d, the density in the caller's units: the stored float, or stored * 0.01f (TEXEL16)."""
    return (stored * f32(0.01)).astype(f32) if fmt == TEXEL16 else stored


def passable(d: np.ndarray) -> np.ndarray:
    """d > 0: NaN, +-0 and negatives are walls."""
    with np.errstate(invalid="ignore"):
        return d > f32(0.0)


def exterior(mask: np.ndarray):
    """(labels, sweeps): the passable samples on a face of the grid and everything 6-connected to them through passable samples;
    sweeps counts the dilations, the last of which changed nothing."""
    ext = np.zeros_like(mask)
    for axis in range(3):
        for face in (0, -1):
            at = [slice(None)] * 3
            at[axis] = face
            ext[tuple(at)] = mask[tuple(at)]
    sweeps = 0
    while True:
        grown = ext.copy()
        for axis in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            grown[tuple(hi)] |= ext[tuple(lo)]
            grown[tuple(lo)] |= ext[tuple(hi)]
        grown &= mask
        sweeps += 1
        if np.array_equal(grown, ext):
            return ext, sweeps
        ext = grown


def fill(stored: np.ndarray, material: np.ndarray, fmt: int, wall: float = 1.0, material_id: int = -1):
    """(stored', material', info): copies with every enclosed sample holding m = -(d + wall) — its texel in TEXEL16 — and, material_id
    >= 0, that id; info = {"filled", "lo", "hi", "sweeps"} with the inclusive xyz box of the written samples (lo > hi when none)."""
    assert fmt in (F32, TEXEL16) and stored.dtype == np.float32 and material.dtype == np.uint8
    N = stored.shape[0]
    d = decode(stored, fmt)
    mask = passable(d)
    ext, sweeps = exterior(mask)
    enclosed = mask & ~ext
    out, mat = stored.copy(), material.copy()
    with np.errstate(all="ignore"):
        m = (-(d + f32(wall))).astype(f32)
    out[enclosed] = (texel16_field(m) if fmt == TEXEL16 else m)[enclosed]
    if material_id >= 0:
        mat[enclosed] = np.uint8(material_id)
    if not enclosed.any():
        return out, mat, {"filled": 0, "lo": (N, N, N), "hi": (-1, -1, -1), "sweeps": sweeps}
    x, z, y = np.nonzero(enclosed)
    info = {"filled": int(enclosed.sum()), "lo": (int(x.min()), int(y.min()), int(z.min())),
            "hi": (int(x.max()), int(y.max()), int(z.max())), "sweeps": sweeps}
    return out, mat, info


# ---- hand-made fields ------------------------------------------------------------------------------------------------------------

N_HAND = 33  # resolution 5: five 8^3 tiles per axis, the last one a single sample thick


def _solid():
    return np.full((N_HAND,) * 3, -1.0, f32)


def _box(d, lo, hi, value):
    """The samples lo..hi (xyz, inclusive) of the [x, z, y] array d."""
    d[lo[0]:hi[0] + 1, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1] = f32(value)


def channel_field():
    """A one-sample-wide channel (0.5) that opens on the face x = 0 and runs back and forth along x at z = 5 — rows y = 3, 7, ..., 27,
    joined at alternating ends —, 21 crossings of a tile border along x and 3 along y; and a sealed 3^3 cavity (0.75) elsewhere."""
    d = _solid()
    rows = list(range(3, 28, 4))
    for k, y in enumerate(rows):
        _box(d, (0 if k == 0 else 2, y, 5), (29, y, 5), 0.5)
        if k + 1 < len(rows):
            x = 29 if k % 2 == 0 else 2
            _box(d, (x, y, 5), (x, y + 4, 5), 0.5)
    _box(d, (20, 20, 20), (22, 22, 22), 0.75)
    return d


def diagonal_field(bridge: int = 0):
    """A region (0.5) that reaches the face x = 0 and a 3^3 cavity (0.25) whose only contact is the cube diagonal between the region's
    corner (10, 12, 12) and the cavity's (11, 13, 13).  bridge = 1 adds (11, 12, 12): 6-connected to the region, in contact with the
    cavity over an edge diagonal.  bridge = 2 adds (11, 13, 12) as well: the contact is 6-connected (a cube diagonal takes two samples
    to bridge)."""
    d = _solid()
    _box(d, (0, 10, 10), (10, 12, 12), 0.5)
    _box(d, (11, 13, 13), (13, 15, 15), 0.25)
    if bridge >= 1:
        _box(d, (11, 12, 12), (11, 12, 12), 0.5)
    if bridge >= 2:
        _box(d, (11, 13, 12), (11, 13, 12), 0.5)
    return d


def odd_walls_field():
    """A 3^3 cavity (0.5) at 14..16 between two channels that reach the faces x = 0 and x = N - 1, closed towards them by one NaN sample
    and one -0.0 sample; two more NaN samples and a +0.0 sample sit elsewhere in its wall."""
    d = _solid()
    _box(d, (14, 14, 14), (16, 16, 16), 0.5)
    _box(d, (0, 15, 15), (12, 15, 15), 0.5)
    _box(d, (18, 15, 15), (N_HAND - 1, 15, 15), 0.5)
    d[13, 15, 15] = np.nan
    d[17, 15, 15] = f32(-0.0)
    d[15, 13, 15] = np.nan   # z = 13
    d[15, 15, 17] = np.nan   # y = 17
    d[15, 17, 14] = f32(0.0)  # z = 17
    return d


def face_field():
    """Cavities that touch a face of the grid on each axis: all exterior."""
    d = _solid()
    _box(d, (0, 10, 10), (2, 12, 12), 0.5)
    _box(d, (10, N_HAND - 3, 20), (12, N_HAND - 1, 22), 0.5)
    _box(d, (20, 20, N_HAND - 1), (22, 22, N_HAND - 1), 0.5)
    _box(d, (N_HAND - 1, 5, 5), (N_HAND - 1, 5, 5), 0.5)
    return d


def two_cavities_field():
    """Two separate 3^3 cavities, in different tiles on every axis."""
    d = _solid()
    _box(d, (5, 6, 7), (7, 8, 9), 0.5)
    _box(d, (25, 20, 15), (27, 22, 17), 1.25)
    return d


def hand_made_fields() -> dict:
    """name -> (density [x, z, y], wall, material, filled, lo, hi): what each field must give (lo / hi None when nothing is filled)."""
    return {
        "channel": (channel_field(), 1.0, 1, 27, (20, 20, 20), (22, 22, 22)),
        "cube diagonal": (diagonal_field(0), 1.0, 1, 27, (11, 13, 13), (13, 15, 15)),
        "edge diagonal": (diagonal_field(1), 1.0, 1, 27, (11, 13, 13), (13, 15, 15)),
        "bridged diagonal": (diagonal_field(2), 1.0, 1, 0, None, None),
        "nan and -0 walls": (odd_walls_field(), 1.0, 7, 27, (14, 14, 14), (16, 16, 16)),
        "cavities on the faces": (face_field(), 1.0, 1, 0, None, None),
        "two cavities": (two_cavities_field(), 1.0, 200, 54, (5, 6, 7), (27, 22, 17)),
        "wall 0, ids untouched": (two_cavities_field(), 0.0, -1, 54, (5, 6, 7), (27, 22, 17)),
    }


def hand_made_material(d: np.ndarray) -> np.ndarray:
    """Ids that tell an untouched sample from a written one: the Voxelizer's (d <= 0) plus a pattern in the upper bits."""
    idx = np.arange(d.size, dtype=np.uint32).reshape(d.shape)
    with np.errstate(invalid="ignore"):
        return ((d <= 0).astype(np.uint8) | ((idx % 5) << 4).astype(np.uint8)).astype(np.uint8)
