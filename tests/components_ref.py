"""Plain-numpy reference of vrt_volume_components, written from the contract in include/vrt.h rather than from either C++ build: whole
[x, z, y] arrays, labels by repeated minimum over the six shifted arrays under the solid mask until nothing changes.  The arithmetic
is np.float32: one negation, one maximum.

The state is what the device stores, as in fill_ref: `stored` is the DENSE buffer (F32: the densities; TEXEL16: the integer field
+-q as float32) and `material` the material ids.  Everything here works from that stored field: a TEXEL16 slot stores 0 for 1e-30, so
there the sample is solid.  components() leaves both arrays alone and returns edited copies.

hand_made_fields() builds the 33^3 fields of tests/test_volume_components*.py: the smallest shapes at which a labelling, its merge
across 8^3 tiles and the edit can go wrong."""
from __future__ import annotations

import numpy as np

from volume_ref import F32, TEXEL16, texel16_field

f32 = np.float32
REPORT, KEEP_LARGEST, REMOVE_SMALL, KEEP_SEED, REMOVE_SEED = range(5)
PASSABLE = np.uint32(0xFFFFFFFF)


class NoSolidSampleAtSeed(Exception):
    """Rule 4: the seed's 3^3 neighbourhood holds no solid sample — the call returns VRT_ERR_INVALID and writes nothing."""


def decode(stored: np.ndarray, fmt: int) -> np.ndarray:
    """d, the density in the caller's units: the stored float, or stored * 0.01f (TEXEL16)."""
    return (stored * f32(0.01)).astype(f32) if fmt == TEXEL16 else stored


def solid(d: np.ndarray) -> np.ndarray:
    """!(d > 0): NaN, +-0 and negatives."""
    with np.errstate(invalid="ignore"):
        return ~(d > f32(0.0))


def _neighbours(a: np.ndarray, fill):
    """The six arrays b with b[p] = a[p +- one step along an axis], `fill` beyond the grid."""
    for axis in range(3):
        for off in (-1, 1):
            b = np.full_like(a, fill)
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            src[axis], dst[axis] = (slice(0, -1), slice(1, None)) if off < 0 else (slice(1, None), slice(0, -1))
            b[tuple(dst)] = a[tuple(src)]
            yield b


def labels_of(mask: np.ndarray) -> np.ndarray:
    """uint32 [x, z, y]: the lowest key (x*N + z)*N + y of every solid sample's 6-connected component, PASSABLE elsewhere."""
    keys = np.arange(mask.size, dtype=np.uint32).reshape(mask.shape)
    lab = np.where(mask, keys, PASSABLE)
    while True:
        low = lab
        for nb in _neighbours(lab, PASSABLE):
            low = np.minimum(low, nb)
        low = np.where(mask, low, PASSABLE)
        if np.array_equal(low, lab):
            return lab
        lab = low


def xyz_of(key: int, N: int):
    return (int(key) // (N * N), int(key) % N, (int(key) // N) % N)


def component_list(lab: np.ndarray):
    """The components in the list order (samples descending, ties by identity ascending): dicts {"key", "first", "lo", "hi", "samples"}."""
    N = lab.shape[0]
    flat = lab.reshape(-1)
    at = np.flatnonzero(flat != PASSABLE)
    if at.size == 0:
        return []
    ids, inverse, counts = np.unique(flat[at], return_inverse=True, return_counts=True)
    coords = {"x": at // (N * N), "y": at % N, "z": (at // N) % N}
    lo, hi = {}, {}
    for a, c in coords.items():
        lo[a] = np.full(ids.size, N, np.int64)
        hi[a] = np.full(ids.size, -1, np.int64)
        np.minimum.at(lo[a], inverse, c)
        np.maximum.at(hi[a], inverse, c)
    order = np.lexsort((ids, -counts.astype(np.int64)))
    return [{"key": int(ids[i]), "first": xyz_of(ids[i], N), "lo": (int(lo["x"][i]), int(lo["y"][i]), int(lo["z"][i])),
             "hi": (int(hi["x"][i]), int(hi["y"][i]), int(hi["z"][i])), "samples": int(counts[i])} for i in order]


def seed_component(lab: np.ndarray, seed) -> int:
    """The label of the solid sample of the seed's 3^3 neighbourhood (clipped) nearest the seed in squared index distance, ties to
    the lowest key."""
    N = lab.shape[0]
    best = None
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                x, y, z = seed[0] + dx, seed[1] + dy, seed[2] + dz
                if min(x, y, z) < 0 or max(x, y, z) >= N or lab[x, z, y] == PASSABLE:
                    continue
                rank = (dx * dx + dy * dy + dz * dz, (x * N + z) * N + y)
                if best is None or rank < best[0]:
                    best = (rank, int(lab[x, z, y]))
    if best is None:
        raise NoSolidSampleAtSeed(tuple(seed))
    return best[1]


def components(stored: np.ndarray, material: np.ndarray, fmt: int, op: int, gap: float = 0.0, material_id: int = -1, min_samples: int = 0,
               seed=(0, 0, 0), list_capacity: int = 0):
    """(stored', material', info): copies after the call; info is what Renderer.components returns (_abi.components_dict): "lo", "hi",
    "written", "solid", "removed_samples", "components", "removed" and "list".  Raises NoSolidSampleAtSeed where the call returns
    VRT_ERR_INVALID after reading the device."""
    assert fmt in (F32, TEXEL16) and stored.dtype == np.float32 and material.dtype == np.uint8
    N = stored.shape[0]
    gap = f32(gap)
    d = decode(stored, fmt)
    mask = solid(d)
    lab = labels_of(mask)
    comps = component_list(lab)
    if op == REPORT:
        gone = set()
    elif op == KEEP_LARGEST:
        gone = {c["key"] for c in comps[1:]}
    elif op == REMOVE_SMALL:
        gone = {c["key"] for c in comps if c["samples"] < min_samples}
    else:
        at_seed = seed_component(lab, seed)
        gone = {c["key"] for c in comps if c["key"] != at_seed} if op == KEEP_SEED else {at_seed}
    removed = mask & np.isin(lab, np.fromiter(gone, np.uint32, len(gone)))
    kept = mask & ~removed
    out, mat = stored.copy(), material.copy()
    # rule 5
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(d), gap, np.maximum(-d, gap)).astype(f32)
    out[removed] = (texel16_field(m) if fmt == TEXEL16 else m)[removed]
    if material_id >= 0:
        mat[removed] = np.uint8(material_id)
    # rule 6, from the field before the call
    by_removed, by_kept = np.zeros_like(mask), np.zeros_like(mask)
    for nb in _neighbours(removed, False):
        by_removed |= nb
    for nb in _neighbours(kept, False):
        by_kept |= nb
    with np.errstate(invalid="ignore"):
        halo = ~mask & (d < gap) & by_removed & ~by_kept
    value = texel16_field(np.full(1, gap, f32))[0] if fmt == TEXEL16 else gap
    halo &= stored.view(np.uint32) != np.array(value, f32).view(np.uint32)
    out[halo] = value
    written = removed | halo
    info = {"lo": (N, N, N), "hi": (-1, -1, -1), "written": int(written.sum()), "solid": int(mask.sum()),
            "removed_samples": int(removed.sum()), "components": len(comps), "removed": len(gone)}
    if written.any():
        x, z, y = np.nonzero(written)
        info["lo"], info["hi"] = (int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max()))
    info["list"] = [{"first": c["first"], "lo": c["lo"], "hi": c["hi"], "removed": int(c["key"] in gone), "samples": c["samples"]}
                    for c in comps[:list_capacity]]
    return out, mat, info


# ---- hand-made fields ------------------------------------------------------------------------------------------------------------

N_HAND = 33  # resolution 5: five 8^3 tiles per axis, the last one a single sample thick


def _empty():
    return np.full((N_HAND,) * 3, 1.0, f32)


def _box(d, lo, hi, value=-1.0):
    """The samples lo..hi (xyz, inclusive) of the [x, z, y] array d."""
    d[lo[0]:hi[0] + 1, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1] = f32(value)


def serpentine_field():
    """fill_ref.channel_field's geometry, solid where that is passable: rows y = 3, 7, ..., 27 at z = 5, x = 2..29 (the first from
    x = 0), joined at alternating ends — 21 crossings of a tile border along x —, and a 3^3 blob at 20..22."""
    d = _empty()
    rows = list(range(3, 28, 4))
    for k, y in enumerate(rows):
        _box(d, (0 if k == 0 else 2, y, 5), (29, y, 5))
        if k + 1 < len(rows):
            x = 29 if k % 2 == 0 else 2
            _box(d, (x, y, 5), (x, y + 4, 5))
    _box(d, (20, 20, 20), (22, 22, 22))
    return d


def arms_field():
    """Two bars inside tile 0 that only meet through tile 1."""
    d = _empty()
    _box(d, (2, 2, 2), (9, 2, 2))
    _box(d, (2, 5, 2), (9, 5, 2))
    _box(d, (9, 2, 2), (9, 5, 2))
    return d


def diagonals_field(bridge: int = 0):
    """Two boxes in contact over a cube diagonal; bridge = 1 adds (11, 12, 12), an edge contact; bridge = 2 adds (11, 13, 12) too."""
    d = _empty()
    _box(d, (0, 10, 10), (10, 12, 12))
    _box(d, (11, 13, 13), (13, 15, 15))
    if bridge >= 1:
        _box(d, (11, 12, 12), (11, 12, 12))
    if bridge >= 2:
        _box(d, (11, 13, 12), (11, 13, 12))
    return d


def odd_values_field():
    """Along x = 10..16 at y = z = 15: -1, NaN, -0.0, +0.0, 1e-30, -1e-30, -inf."""
    d = _empty()
    for x, value in zip(range(10, 17), (-1.0, np.nan, -0.0, 0.0, 1e-30, -1e-30, -np.inf)):
        d[x, 15, 15] = f32(value)
    return d


def ties_field():
    d = _empty()
    _box(d, (5, 6, 7), (7, 8, 9))
    _box(d, (25, 20, 15), (27, 22, 17))
    return d


HALO_BETWEEN = [(x, y, 7) for x in (7, 8, 9) for y in (7, 8, 9)]  # touch the slab and the blob
HALO_FAR = (10, 8, 9)  # a 6-neighbour of the blob at 0.75: not below the gap


def halo_field():
    """A slab (4..12, 4..12, 4..6) that stays and a 3^3 blob (7..9, 7..9, 8..10) one passable sample above it in z; every passable
    sample within one step (diagonals included) of a solid one holds 0.25, the blob's neighbour HALO_FAR 0.75."""
    d = _empty()
    _box(d, (4, 4, 4), (12, 12, 6))
    _box(d, (7, 7, 8), (9, 9, 10))
    s = d < 0
    near = np.zeros_like(s)
    p = np.pad(s, 1)
    for dx in range(3):
        for dz in range(3):
            for dy in range(3):
                near |= p[dx:dx + N_HAND, dz:dz + N_HAND, dy:dy + N_HAND]
    d[near & ~s] = f32(0.25)
    d[HALO_FAR[0], HALO_FAR[2], HALO_FAR[1]] = f32(0.75)
    return d


def checkerboard_field():
    x, z, y = np.indices((N_HAND,) * 3)
    return np.where((x + y + z) % 2 == 0, f32(-1.0), f32(0.25)).astype(f32)


def faces_field():
    d = _empty()
    _box(d, (0, 0, 0), (0, 0, 0))
    _box(d, (32, 32, 32), (32, 32, 32))
    _box(d, (32, 28, 32), (32, 30, 32))
    return d


def hand_made_fields() -> dict:
    """name -> (density [x, z, y], components in F32 as [(samples, first)], the same in TEXEL16)."""
    n3 = N_HAND ** 3
    plain = {
        "serpentine": (serpentine_field(), [(216, (0, 3, 5)), (27, (20, 20, 20))]),
        "arms": (arms_field(), [(18, (2, 2, 2))]),
        "diagonals": (diagonals_field(0), [(99, (0, 10, 10)), (27, (11, 13, 13))]),
        "diagonals, edge": (diagonals_field(1), [(100, (0, 10, 10)), (27, (11, 13, 13))]),
        "diagonals, bridged": (diagonals_field(2), [(128, (0, 10, 10))]),
        "ties": (ties_field(), [(27, (5, 6, 7)), (27, (25, 20, 15))]),
        "halo": (halo_field(), [(243, (4, 4, 4)), (27, (7, 7, 8))]),
        "faces": (faces_field(), [(3, (32, 28, 32)), (1, (0, 0, 0)), (1, (32, 32, 32))]),
        "all passable": (_empty(), []),
        "all solid": (np.full((N_HAND,) * 3, -1.0, f32), [(n3, (0, 0, 0))]),
    }
    out = {name: (d, want, want) for name, (d, want) in plain.items()}
    out["odd values"] = (odd_values_field(), [(4, (10, 15, 15)), (2, (15, 15, 15))], [(7, (10, 15, 15))])
    board = checkerboard_field()
    firsts = [xyz_of(k, N_HAND) for k in np.flatnonzero(board.reshape(-1) < 0)]
    out["checkerboard"] = (board, [(1, f) for f in firsts], [(1, f) for f in firsts])
    return out


def hand_made_records() -> dict:
    """name -> the records each field is edited with, as keyword arguments of components(): every op that applies to it."""
    n3 = N_HAND ** 3
    two = [dict(op=KEEP_LARGEST, gap=0.5, material_id=0), dict(op=REMOVE_SMALL, gap=0.25, material_id=9, min_samples=28),
           dict(op=REMOVE_SMALL, gap=0.5, min_samples=1000)]
    return {
        "serpentine": two + [dict(op=REMOVE_SEED, gap=0.5, material_id=3, seed=(16, 7, 5)), dict(op=KEEP_SEED, gap=0.5, seed=(21, 21, 21))],
        "arms": [dict(op=KEEP_LARGEST, gap=0.5), dict(op=REMOVE_SEED, gap=0.5, material_id=0, seed=(2, 5, 2))],
        "diagonals": two,
        "diagonals, edge": two,
        "diagonals, bridged": two,
        "odd values": [dict(op=REMOVE_SMALL, gap=0.5, material_id=2, min_samples=3), dict(op=KEEP_LARGEST, gap=2.0),
                       dict(op=REMOVE_SMALL, gap=0.25, material_id=0, min_samples=8)],
        "ties": [dict(op=KEEP_LARGEST, gap=0.5, material_id=0), dict(op=KEEP_SEED, gap=0.5, material_id=0, seed=(24, 19, 14)),
                 dict(op=REMOVE_SEED, gap=0.5, seed=(8, 9, 10))],
        "halo": [dict(op=KEEP_LARGEST, gap=0.5, material_id=0), dict(op=REMOVE_SEED, gap=0.5, seed=(8, 8, 9))],
        "checkerboard": [dict(op=REMOVE_SMALL, gap=0.5, material_id=0, min_samples=2), dict(op=KEEP_LARGEST, gap=0.125)],
        "faces": [dict(op=KEEP_LARGEST, gap=0.5, material_id=0), dict(op=REMOVE_SMALL, gap=0.5, min_samples=2),
                  dict(op=KEEP_SEED, gap=0.5, seed=(31, 31, 31)), dict(op=REMOVE_SEED, gap=0.5, seed=(0, 0, 0))],
        "all passable": [dict(op=KEEP_LARGEST, gap=0.5), dict(op=REMOVE_SMALL, gap=0.5, min_samples=5)],
        "all solid": [dict(op=KEEP_LARGEST, gap=0.5), dict(op=REMOVE_SMALL, gap=0.5, material_id=0, min_samples=n3 + 1)],
    }


def specks_field(N: int = 257, specks: int = 300, seed: int = 257):
    """(density, material) of the large case: the signed distance to a sphere of 60 cells inside the block of samples within 72 cells
    of its centre on each axis, 30 elsewhere, and some `specks` seeded specks of one to three solid samples (-0.5) outside that block —
    40 of them in the last x planes, beyond lane 2^24 of a launch capped at 65 536 workgroups of 256 —, each with a passable
    neighbour below a gap of 0.5."""
    centre, radius, reach = (N // 2, N // 2 - 2, N // 2 + 2), 60.0, 72
    d = np.full((N,) * 3, 30.0, f32)
    x, z, y = (np.arange(c - reach, c + reach + 1, dtype=np.float64) for c in (centre[0], centre[2], centre[1]))
    block = np.sqrt((x[:, None, None] - centre[0]) ** 2 + (y[None, None, :] - centre[1]) ** 2 + (z[None, :, None] - centre[2]) ** 2) - radius
    d[x[0].astype(int):x[-1].astype(int) + 1, z[0].astype(int):z[-1].astype(int) + 1, y[0].astype(int):y[-1].astype(int) + 1] = block.astype(f32)
    rng = np.random.default_rng(seed)
    at = rng.integers(1, N - 3, (specks, 3))
    at[:40, 0] = rng.integers(N - 4, N - 1, 40)
    at = at[(np.abs(at - N // 2) > reach + 4).any(axis=1)]  # clear of the sphere's block
    for n, (px, py, pz) in enumerate(at):
        d[px, pz, py:py + 1 + n % 3] = f32(-0.5)
        if d[px + 1, pz, py] > 0:
            d[px + 1, pz, py] = f32(0.1)
    with np.errstate(invalid="ignore"):
        return d, (d <= 0).astype(np.uint8)


TIES_NO_SOLID_SEED = (9, 10, 11)  # two samples away, on every axis, from the nearest blob of ties_field()


def hand_made_material(d: np.ndarray) -> np.ndarray:
    """Ids that tell an untouched sample from a written one: the Voxelizer's (d <= 0) plus a pattern in the upper bits."""
    idx = np.arange(d.size, dtype=np.uint32).reshape(d.shape)
    with np.errstate(invalid="ignore"):
        return ((d <= 0).astype(np.uint8) | ((idx % 5) << 4).astype(np.uint8)).astype(np.uint8)
