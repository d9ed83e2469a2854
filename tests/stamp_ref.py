"""Plain-numpy reference of vrt_volume_stamp, written from the contract in include/vrt.h rather than from the kernel: whole [x, z, y]
arrays, every sample of the destination grid, no footprint box.  Every operation is an np.float32 operation in the header's
parenthesisation (numpy's ufuncs round once per operation and never fuse a multiply with an add).

The state is what the device stores: `stored` is the DENSE buffer (F32: the densities; TEXEL16: the integer field +-q as float32)
and `material` the material ids, of the destination and of the source.  apply() edits the destination in place and returns what
vrt_brush_result reports."""
from __future__ import annotations

import numpy as np

from brush_ref import decode, units
from volume_ref import F32, TEXEL16, texel16_field

ADD, SUBTRACT, REPLACE = 0, 1, 2
KEEP, SOURCE = -1, -2
f32 = np.float32


def source_coords(matrix, N: int):
    """Step 1: (ux, uy, uz) at every destination sample, float32 [x, z, y] each; matrix: 12 values, row-major 3x4."""
    M = np.asarray(matrix, dtype=f32).reshape(3, 4)
    i = np.arange(N, dtype=f32)
    full = lambda v: np.ascontiguousarray(np.broadcast_to(v, (N, N, N)), dtype=f32)
    px, pz, py = full(i[:, None, None]), full(i[None, :, None]), full(i[None, None, :])
    with np.errstate(all="ignore"):
        return tuple(((M[a, 0] * px + M[a, 1] * py) + M[a, 2] * pz) + M[a, 3] for a in range(3))


def lerp(s0, s1, f):
    return (s0 * (f32(1.0) - f)) + (s1 * f)


def sample_source(src_stored, src_material, src_fmt: int, matrix, N: int):
    """Steps 1-4: (inside mask, t, nearest source material id) at every destination sample; t and the id are meaningless outside."""
    Ns = src_stored.shape[0]
    u = source_coords(matrix, N)  # x, y, z
    last = f32(Ns - 1)
    with np.errstate(all="ignore"):
        inside = np.ones((N, N, N), bool)
        for ua in u:
            inside &= (ua >= f32(0.0)) & (ua <= last)
        cell, frac = [], []
        for ua in u:
            safe = np.where(inside, ua, f32(0.0))
            c = np.minimum(np.maximum(np.floor(safe).astype(np.int64), 0), Ns - 2)
            cell.append(c)
            frac.append((safe - c.astype(f32)).astype(f32))
        (cx, cy, cz), (fx, fy, fz) = cell, frac
        s = decode(np.asarray(src_stored, f32), src_fmt)  # [x, z, y]
        tap = lambda dx, dy, dz: s[cx + dx, cz + dz, cy + dy]
        c00, c10 = lerp(tap(0, 0, 0), tap(1, 0, 0), fx), lerp(tap(0, 1, 0), tap(1, 1, 0), fx)
        c01, c11 = lerp(tap(0, 0, 1), tap(1, 0, 1), fx), lerp(tap(0, 1, 1), tap(1, 1, 1), fx)
        t = lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz).astype(f32)
    near = lambda c, f: c + (f >= f32(0.5))
    ids = np.asarray(src_material, np.uint8)[near(cx, fx), near(cz, fz), near(cy, fy)]
    return inside, t, ids


def apply(stored, material, fmt: int, extent: float, density_scale: float, src_stored, src_material, src_fmt: int, src_extent: float,
          src_density_scale: float, rec) -> dict:
    """The record on the whole destination, in place.  rec: op, material, dst_to_src (12), length_scale, offset, blend, reach (a
    vrt_stamp or anything shaped like one).  Returns {"written", "lo", "hi"}: the samples written and their inclusive xyz box
    (lo > hi when none)."""
    assert fmt in (F32, TEXEL16) and src_fmt in (F32, TEXEL16) and stored.dtype == np.float32 and material.dtype == np.uint8
    N, Ns = stored.shape[0], src_stored.shape[0]
    _, unit_dst = units(N, extent, density_scale)
    _, unit_src = units(Ns, src_extent, src_density_scale)
    gain = f32(f32(f32(rec.length_scale) * unit_dst) / unit_src)
    off, k, rv = f32(f32(rec.offset) * unit_dst), f32(f32(rec.blend) * unit_dst), f32(f32(rec.reach) * unit_dst)
    inside, t, ids = sample_source(src_stored, src_material, src_fmt, list(rec.dst_to_src), N)
    d = decode(stored, fmt)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        v = ((t * gain) - off).astype(f32)
        if rec.op == REPLACE:
            m, w = v, v == v
        elif rec.op == ADD:
            m = np.fmin(d, v)
            if k > 0:
                g = np.fmax(k - np.abs(d - v), zero) / k
                m = m - ((g * g) * k) * f32(0.25)
            w = (v < rv) & (m < d)
        else:
            assert rec.op == SUBTRACT
            c = -v
            m = np.fmax(d, c)
            if k > 0:
                g = np.fmax(k - np.abs(d - c), zero) / k
                m = m + ((g * g) * k) * f32(0.25)
            w = (v < rv) & (m > d)
        m = m.astype(f32)
        w = w & inside
        solid = m <= zero
    stored[w] = (texel16_field(m) if fmt == TEXEL16 else m)[w]
    if rec.material >= 0:
        material[w] = np.where(solid, np.uint8(rec.material), np.uint8(0))[w]
    elif rec.material == SOURCE:
        material[w] = (ids if rec.op == REPLACE else np.where(solid, ids, np.uint8(0)))[w]
    else:
        assert rec.material == KEEP
    if not w.any():
        return {"written": 0, "lo": (N, N, N), "hi": (-1, -1, -1)}
    x, z, y = np.nonzero(w)
    return {"written": int(w.sum()), "lo": (int(x.min()), int(y.min()), int(z.min())), "hi": (int(x.max()), int(y.max()), int(z.max()))}
