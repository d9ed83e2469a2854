"""Plain-numpy reference of every device buffer an upload builds (vrt_debug_volume_bytes), written from the definitions in
vrt.h and vrt_device.h rather than from the kernels: the dense grid (fp32, or the TEXEL16 integer field +-q), the materials, the
bricks, the cell records, both levels of the empty-space table, the Cube modes' table and the active box.

Arrays are indexed [x, z, y] like the grid; brick (bx, bz, by) is record (bx*nb + bz)*nb + by.  Every product that decides a
table entry is an np.float32 product with the kernels' operand order (sample * scale)."""
from __future__ import annotations

import numpy as np

F32, TEXEL16 = 0, 1
NIB_CAP = 15       # a sub-block nibble holds at most 15 (cells)
NIB_WINDOW = 16    # per-axis cell offset to an active cell the level-2 reference searches: offset 16 is a gap of 15 cells, whose
                   # square, 225, already gives the capped nibble, so a wider window changes nothing (a narrower one does)
NO_NEAR = 255      # brick distance of "no seed anywhere"


def n_bricks(N: int) -> int:
    return (N - 1 + 3) // 4


# ---- the TEXEL16 quantiser (VRT_FORMAT_TEXEL16) -------------------------------------------------------------------------

def texel16_q(d) -> np.ndarray:
    """q of the 16-bit texel: trunc(|d| * 100) in fp32, saturated to 0xffffffff when |d| * 100 >= 4294967040 (the largest fp32
    below 2^32; inf included), 0 for NaN, then the low 15 bits.  uint32, the shape of d."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):  # inf / NaN in, by design
        a = np.abs(d) * np.float32(100.0)
    sat = a >= np.float32(4294967040.0)
    ok = (a >= np.float32(0.0)) & ~sat  # NaN compares false
    q = np.zeros(d.shape, np.uint64)
    q[ok] = a[ok].astype(np.uint64)     # trunc, exact below 2^32
    q[sat] = 0xFFFFFFFF
    return (q & 0x7FFF).astype(np.uint32)


def texel16_field(d) -> np.ndarray:
    """The integer field +-q as float32: -q where d < 0 (-0.0 when q is 0), else q."""
    d = np.asarray(d, dtype=np.float32)
    q = texel16_q(d).astype(np.float32)
    return np.where(d < 0, -q, q).astype(np.float32)


def decode_texels(tex) -> tuple:
    """The reference's RGBA8 volume texture (uint8 [z, y, x, 4]; R = sign<<7 | q>>8, G = q & 0xff, B = material) ->
    (field +-q float32 [x, z, y], material uint8 [x, z, y]), byte by byte."""
    tex = np.asarray(tex, dtype=np.uint8)
    r = tex[..., 0].astype(np.uint32)
    g = tex[..., 1].astype(np.uint32)
    q = (((r & 0x7F) << 8) | g).astype(np.float32)
    field = np.where((r & 0x80) != 0, -q, q).astype(np.float32)
    to_xzy = lambda a: np.ascontiguousarray(np.transpose(a, (2, 0, 1)))  # [z, y, x] -> [x, z, y]
    return to_xzy(field), to_xzy(tex[..., 2])


def split_records(rec) -> tuple:
    """VVoxel records {u8 material, pad[3], f32 density} -> (density bits as float32, material)."""
    raw = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 8)
    return raw[:, 4:8].copy().view(np.float32).reshape(-1), raw[:, 0].copy()


def dense_field(density, fmt: int) -> np.ndarray:
    """What DENSE holds after vrt_volume_upload / _upload_voxels of `density` in format fmt."""
    d = np.asarray(density, dtype=np.float32)
    return texel16_field(d) if fmt == TEXEL16 else d.copy()


def scale_of(fmt: int, density_scale: float) -> np.float32:
    """The factor a dense sample is multiplied by before the step clamp: density_scale, times 0.01f in TEXEL16."""
    s = np.float32(density_scale)
    return np.float32(s * np.float32(0.01)) if fmt == TEXEL16 else s


def near_samples(dense, s, step_max) -> np.ndarray:
    """Samples below the step clamp: dense * s < step_max (strict; NaN never)."""
    return np.asarray(dense, np.float32) * np.float32(s) < np.float32(step_max)


# ---- bricks and cell records ---------------------------------------------------------------------------------------------

def _brick_ids(nb: int, which):
    ids = np.arange(nb ** 3, dtype=np.int64) if which is None else np.asarray(which, dtype=np.int64).reshape(-1)
    return ids, ids // (nb * nb), (ids // nb) % nb, ids % nb


def bricks(dense, fmt: int, which=None, chunk: int = 8192) -> np.ndarray:
    """Brick records [n, 128] (float32 for F32, int16 for TEXEL16) of all bricks or of the brick ids `which`: sample (lx, lz, ly)
    of a brick at lane lx*25 + lz*5 + ly, from voxel (4bx + lx, 4bz + lz, 4by + ly) clamped to N-1; lanes 125-127 hold 0."""
    dense = np.asarray(dense, np.float32)
    N = dense.shape[0]
    ids, bx, bz, by = _brick_ids(n_bricks(N), which)
    lane = np.arange(125)
    lx, lz, ly = lane // 25, (lane // 5) % 5, lane % 5
    out = np.zeros((ids.size, 128), np.int16 if fmt == TEXEL16 else np.float32)
    for a in range(0, ids.size, chunk):
        b = slice(a, a + chunk)
        x = np.minimum(bx[b, None] * 4 + lx, N - 1)
        z = np.minimum(bz[b, None] * 4 + lz, N - 1)
        y = np.minimum(by[b, None] * 4 + ly, N - 1)
        v = dense[x, z, y]
        out[b, :125] = v.astype(np.int16) if fmt == TEXEL16 else v
    return out


def cells(dense, which=None, chunk: int = 8192) -> np.ndarray:
    """TEXEL16 cell records [n, 64, 8] int16: record lx*16 + lz*4 + ly of a brick holds the 8 corners of cell
    (4bx + lx, 4bz + lz, 4by + ly), tap k = (x, z) 00, 01, 10, 11 with y then y + 1, i.e. offsets (k>>2, (k>>1)&1, k&1);
    coordinates clamped to N-1."""
    dense = np.asarray(dense, np.float32)
    N = dense.shape[0]
    ids, bx, bz, by = _brick_ids(n_bricks(N), which)
    rec = np.arange(64)
    k = np.arange(8)
    cx = (rec // 16)[:, None] + (k >> 2)[None, :]           # [64, 8]
    cz = ((rec // 4) % 4)[:, None] + ((k >> 1) & 1)[None, :]
    cy = (rec % 4)[:, None] + (k & 1)[None, :]
    out = np.zeros((ids.size, 64, 8), np.int16)
    for a in range(0, ids.size, chunk):
        b = slice(a, a + chunk)
        x = np.minimum(bx[b, None, None] * 4 + cx, N - 1)
        z = np.minimum(bz[b, None, None] * 4 + cz, N - 1)
        y = np.minimum(by[b, None, None] * 4 + cy, N - 1)
        out[b] = dense[x, z, y].astype(np.int16)
    return out


# ---- level 1: near bricks, Chebyshev distance, active box ---------------------------------------------------------------

def _window_any(m, nb: int, axis: int, apron: bool = True) -> np.ndarray:
    """Along one axis: brick b is set when one of the samples 4b .. 4b+4 is (4b .. 4b+3 without the apron).  The axis holds
    4nb + 1 samples (padded by repeating the last one, i.e. clamped)."""
    m = np.moveaxis(m, axis, 0)
    body = m[:4 * nb].reshape((nb, 4) + m.shape[1:]).any(axis=1)
    if apron:
        body = body | m[4:4 * nb + 1:4]
    return np.moveaxis(body, 0, axis)


def near_bricks(dense, s, step_max, apron: bool = True) -> np.ndarray:
    """bool [nb, nb, nb]: one of the brick's 5^3 clamped samples is below the clamp."""
    m = near_samples(dense, s, step_max)
    N = m.shape[0]
    nb = n_bricks(N)
    pad = 4 * nb + 1 - N
    if pad > 0:
        m = np.pad(m, ((0, pad),) * 3, mode="edge")
    for axis in range(3):
        m = _window_any(m, nb, axis, apron)
    return m


def chebyshev(seeds) -> np.ndarray:
    """uint8 [nb, nb, nb]: Chebyshev distance, in bricks, to the nearest seed; 255 without a seed.  Separable: the L-inf
    distance is min over q of max(|p - q|, D(q)) along each axis in turn."""
    seeds = np.asarray(seeds, bool)
    if not seeds.any():
        return np.full(seeds.shape, NO_NEAR, np.uint8)
    D = np.where(seeds, 0, 1 << 20).astype(np.int32)
    for axis in range(3):
        n = D.shape[axis]
        gap = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.int32)  # [p, q]
        Dm = np.moveaxis(D, axis, -1)                                                  # [..., q]
        D = np.moveaxis(np.maximum(gap, Dm[..., None, :]).min(axis=-1), -1, axis)
    return np.minimum(D, NO_NEAR).astype(np.uint8)


def leap(D) -> np.ndarray:
    """The level-1 buffer: max(D - 1, 0)."""
    return np.maximum(np.asarray(D, np.int32) - 1, 0).astype(np.uint8)


def active_box(near) -> np.ndarray:
    """{min x, z, y, max x, z, y} of the near bricks; {nb, nb, nb, -1, -1, -1} without one."""
    near = np.asarray(near, bool)
    nb = near.shape[0]
    if not near.any():
        return np.array([nb] * 3 + [-1] * 3, np.int32)
    idx = np.nonzero(near)
    return np.array([a.min() for a in idx] + [a.max() for a in idx], np.int32)


# ---- level 2: active cells, sub-block nibbles ----------------------------------------------------------------------------

def active_cells(dense, s, step_max) -> np.ndarray:
    """bool [C, C, C], C = N-1: one of the cell's 8 corners is below the clamp."""
    m = near_samples(dense, s, step_max)
    C = m.shape[0] - 1
    act = np.zeros((C, C, C), bool)
    for dx in (0, 1):
        for dz in (0, 1):
            for dy in (0, 1):
                act |= m[dx:dx + C, dz:dz + C, dy:dy + C]
    return act


def _shift(a, off: int, axis: int, fill):
    """a shifted by off along axis: out[p] = a[p + off], `fill` beyond the ends."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(off) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(off, 0), n + min(off, 0))
    dst[axis] = slice(max(-off, 0), n - max(off, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def cell_d2(act, window: int = NIB_WINDOW) -> np.ndarray:
    """int32 [C, C, C]: squared cube-to-cube distance sum max(|d| - 1, 0)^2 to the nearest active cell, capped at NIB_CAP^2 + 1.
    Computed as the exact squared Euclidean distance to the active set dilated by one cell (3x3x3), searched up to `window` - 1
    cells along each axis."""
    act = np.asarray(act, bool)
    cap = NIB_CAP * NIB_CAP + 1
    dil = act.copy()
    for axis in range(3):
        dil = dil | _shift(dil, 1, axis, False) | _shift(dil, -1, axis, False)
    d2 = np.where(dil, 0, cap).astype(np.int32)
    for axis in range(3):
        best = d2.copy()
        for off in range(1, window):
            for o in (off, -off):
                best = np.minimum(best, _shift(d2, o, axis, cap) + off * off)
        d2 = np.minimum(best, cap)
    return d2


def nibbles(act, window: int = NIB_WINDOW) -> np.ndarray:
    """uint32 [nb, nb, nb]: per brick eight 4-bit fields, sub-block (sx, sz, sy) at bit 4*(sx*4 + sz*2 + sy), each the minimum over
    the sub-block's cells of min(15, floor(sqrt(d2))); cells at C and beyond count as 15."""
    d2 = cell_d2(act, window)
    C = d2.shape[0]
    nb = n_bricks(C + 1)
    r = np.minimum(np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64), NIB_CAP)
    full = np.full((4 * nb,) * 3, NIB_CAP, np.int64)
    full[:C, :C, :C] = r
    e = full.reshape(nb, 2, 2, nb, 2, 2, nb, 2, 2).min(axis=(2, 5, 8))  # [bx, sx, bz, sz, by, sy]
    w = np.zeros((nb, nb, nb), np.uint32)
    for sx in (0, 1):
        for sz in (0, 1):
            for sy in (0, 1):
                w |= e[:, sx, :, sz, :, sy].astype(np.uint32) << np.uint32(4 * (sx * 4 + sz * 2 + sy))
    return w


# ---- the Cube modes' table -------------------------------------------------------------------------------------------------

def cube_seeds(dense) -> np.ndarray:
    """bool [nb, nb, nb]: one of the brick's 4^3 cell-origin voxels with coordinates <= N-2 holds density <= 0 (+-0 does, NaN not)."""
    dense = np.asarray(dense, np.float32)
    N = dense.shape[0]
    C, nb = N - 1, n_bricks(N)
    solid = np.zeros((4 * nb,) * 3, bool)
    solid[:C, :C, :C] = dense[:C, :C, :C] <= 0
    return solid.reshape(nb, 4, nb, 4, nb, 4).any(axis=(1, 3, 5))


# ---- everything at once ------------------------------------------------------------------------------------------------------

def tables(dense, fmt: int, density_scale: float, step_max: float) -> dict:
    """The tables of a DENSE field: 'D' (level-1 Chebyshev distances) and 'skip', 'nib', 'active_box' — None without a bounded
    step (step_max <= 0) — and 'cube_D' = 'cube_skip'."""
    out = {"cube_skip": chebyshev(cube_seeds(dense))}
    if not step_max > 0:
        out.update(D=None, skip=None, nib=None, active_box=None)
        return out
    s = scale_of(fmt, density_scale)
    near = near_bricks(dense, s, step_max)
    D = chebyshev(near)
    out.update(D=D, skip=leap(D), nib=nibbles(active_cells(dense, s, step_max)), active_box=active_box(near))
    return out


def device_bytes(dense, material, fmt: int, density_scale: float, step_max: float, which=None) -> dict:
    """What vrt_debug_volume_bytes returns for a slot holding DENSE field `dense` and `material`, as uint8 arrays ('active_box'
    None without the tables).  which: brick ids to restrict 'bricks' / 'cells' to (their records only, in that order)."""
    dense = np.ascontiguousarray(dense, np.float32)
    t = tables(dense, fmt, density_scale, step_max)
    empty = np.zeros(0, np.uint8)
    as_bytes = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return {
        "dense": as_bytes(dense),
        "material": as_bytes(np.asarray(material, np.uint8)),
        "bricks": as_bytes(bricks(dense, fmt, which)),
        "cells": as_bytes(cells(dense, which)) if fmt == TEXEL16 else empty,
        "skip": as_bytes(t["skip"]) if t["skip"] is not None else empty,
        "nib": as_bytes(t["nib"]) if t["nib"] is not None else empty,
        "cube_skip": as_bytes(t["cube_skip"]),
        "active_box": as_bytes(t["active_box"]) if t["active_box"] is not None else None,
    }
