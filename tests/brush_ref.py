"""Plain-numpy reference of vrt_volume_apply_brushes, written from the contract in include/vrt.h rather than from the kernel: whole
[x, z, y] arrays, the whole volume, no footprint box.  Every operation is an np.float32 operation in the header's parenthesisation
(numpy's ufuncs round once per operation and never fuse a multiply with an add; sqrt and division are correctly rounded).

The state is what the device stores: `stored` is the DENSE buffer (F32: the densities; TEXEL16: the integer field +-q as float32)
and `material` the material ids.  apply() edits both in place and returns what vrt_brush_result reports."""
from __future__ import annotations

import numpy as np

from volume_ref import F32, TEXEL16, texel16_field

SPHERE, BOX, CAPSULE = 0, 1, 2
ADD, SUBTRACT, PAINT = 0, 1, 2
f32 = np.float32


def units(N: int, extent: float, density_scale: float):
    """(cell, unit): cell = (extent * 2.0f) / (float)(N - 1); unit = cell / density_scale."""
    cell = f32(f32(extent) * f32(2.0)) / f32(N - 1)
    return f32(cell), f32(cell / f32(density_scale))


def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def _len(ux, uy, uz):
    return np.sqrt(_dot(ux, uy, uz, ux, uy, uz))


def brush_distance(rec, N: int) -> np.ndarray:
    """s of the record at every sample, float32 [x, z, y]; a and b are (x, y, z)."""
    i = np.arange(N, dtype=f32)
    px, pz, py = i[:, None, None], i[None, :, None], i[None, None, :]
    a = [f32(v) for v in rec.a]
    b = [f32(v) for v in rec.b]
    r = f32(rec.radius)
    zero, one = f32(0.0), f32(1.0)
    full = lambda v: np.broadcast_to(v, (N, N, N)).astype(f32)
    with np.errstate(all="ignore"):
        pax, pay, paz = full(px - a[0]), full(py - a[1]), full(pz - a[2])
        if rec.shape == SPHERE:
            return (_len(pax, pay, paz) - r).astype(f32)
        if rec.shape == CAPSULE:
            bax, bay, baz = f32(b[0] - a[0]), f32(b[1] - a[1]), f32(b[2] - a[2])
            h = np.fmin(np.fmax(_dot(pax, pay, paz, bax, bay, baz) / _dot(bax, bay, baz, bax, bay, baz), zero), one)
            return (_len(pax - bax * h, pay - bay * h, paz - baz * h) - r).astype(f32)
        qx, qy, qz = (np.abs(pax) - b[0]) + r, (np.abs(pay) - b[1]) + r, (np.abs(paz) - b[2]) + r
        outside = _len(np.fmax(qx, zero), np.fmax(qy, zero), np.fmax(qz, zero))
        return ((outside + np.fmin(np.fmax(qx, np.fmax(qy, qz)), zero)) - r).astype(f32)


def decode(stored: np.ndarray, fmt: int) -> np.ndarray:
    """d, the density in the caller's units: the stored float, or stored * 0.01f (TEXEL16)."""
    return (stored * f32(0.01)).astype(f32) if fmt == TEXEL16 else stored


def apply_one(stored: np.ndarray, material: np.ndarray, fmt: int, rec, unit) -> np.ndarray:
    """One record on the whole volume, in place; returns the mask of the samples it wrote."""
    N = stored.shape[0]
    s = brush_distance(rec, N)
    d = decode(stored, fmt)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        if rec.op == PAINT:
            w = (s <= zero) & (d <= zero) & (material != np.uint8(rec.material))
            material[w] = np.uint8(rec.material)
            return w
        v = s * f32(unit)
        k = f32(f32(rec.blend) * f32(unit))
        if rec.op == ADD:
            m = np.fmin(d, v)
            if k > 0:
                g = np.fmax(k - np.abs(d - v), zero) / k
                m = m - ((g * g) * k) * f32(0.25)
            w = (s < f32(rec.reach)) & (m < d)
        else:
            c = -v
            m = np.fmax(d, c)
            if k > 0:
                g = np.fmax(k - np.abs(d - c), zero) / k
                m = m + ((g * g) * k) * f32(0.25)
            w = (s < f32(rec.reach)) & (m > d)
    m = m.astype(f32)
    stored[w] = (texel16_field(m) if fmt == TEXEL16 else m)[w]
    if rec.material >= 0:
        material[w] = np.where(m <= zero, np.uint8(rec.material), np.uint8(0))[w]
    return w


def apply(stored: np.ndarray, material: np.ndarray, fmt: int, records, extent: float, density_scale: float) -> dict:
    """The records in order, in place.  Returns {"written", "lo", "hi"}: the samples written at least once and their inclusive xyz
    box (lo > hi when none)."""
    assert fmt in (F32, TEXEL16) and stored.dtype == np.float32 and material.dtype == np.uint8
    N = stored.shape[0]
    _, unit = units(N, extent, density_scale)
    any_w = np.zeros(stored.shape, bool)
    for rec in records:
        any_w |= apply_one(stored, material, fmt, rec, unit)
    if not any_w.any():
        return {"written": 0, "lo": (N, N, N), "hi": (-1, -1, -1)}
    x, z, y = np.nonzero(any_w)
    return {"written": int(any_w.sum()), "lo": (int(x.min()), int(y.min()), int(z.min())), "hi": (int(x.max()), int(y.max()), int(z.max()))}


def texels_of(stored: np.ndarray, material: np.ndarray) -> np.ndarray:
    """The RGBA8 volume texture (uint8 [z, y, x, 4]) of a TEXEL16 field +-q and its material ids: R = sign<<7 | q>>8, G = q & 0xff,
    B = A = material — what vrt_volume_upload_texels takes, so the field is uploaded without a second quantisation."""
    q = np.abs(stored).astype(np.uint16)
    sign = np.signbit(stored)
    N = stored.shape[0]
    tex = np.zeros((N, N, N, 4), np.uint8)
    r = (q >> 8).astype(np.uint8) | np.where(sign, 0x80, 0).astype(np.uint8)
    for ch, a in ((0, r), (1, (q & 0xFF).astype(np.uint8)), (2, material), (3, material)):
        tex[..., ch] = np.transpose(a, (1, 2, 0))  # [x, z, y] -> [z, y, x]
    return tex
