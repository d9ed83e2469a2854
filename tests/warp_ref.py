"""Plain-numpy reference of vrt_volume_warp, written from the contract in include/vrt.h rather than from the kernels: whole [x, z, y]
arrays, the whole volume, no box.  Every operation is an np.float32 operation in the header's parenthesisation (numpy's ufuncs round
once per operation and never fuse a multiply with an add; sqrt and division are correctly rounded); the clamps are np.fmin / np.fmax,
which drop a NaN as fminf / fmaxf do.

The state is what the device stores: `stored` is the DENSE buffer (F32: the densities; TEXEL16: the integer field +-q as float32)
and `material` the material ids.  warp() leaves both alone and returns the edited copies with what vrt_brush_result reports and the
count of density writes.

Also an in-place variant (what a kernel that wrote straight into the volume, sample after sample in storage order, would leave: only
there to prove that a case can tell it from the rule's Jacobi reads) and what the rule is measured with (tools/warp_probe.py, and one
test of the reference itself): an analytic sphere, warped, and the radial error of its zero crossings against the moved sphere."""
from __future__ import annotations

import numpy as np

from brush_ref import brush_distance, decode, units
from smooth_ref import crossing_errors, noisy_sphere
from stamp_ref import lerp, source_coords
from volume_ref import F32, TEXEL16, texel16_field

KEEP, SOURCE = -1, -2
f32 = np.float32
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def weights(rec, N: int):
    """Step 1: (region mask, w) over the grid; w is 0 outside the region (where nothing reads it)."""
    s = brush_distance(rec, N)
    with np.errstate(all="ignore"):
        region = s < f32(0.0)
        t = np.fmin((-s) / f32(rec.falloff), f32(1.0))
        h = (t * t) * (f32(3.0) - (f32(2.0) * t))
        w = f32(rec.strength) * h
    return region, np.where(region, w, f32(0.0)).astype(f32)


def geometry(rec, N: int, unit) -> dict:
    """Everything of steps 1, 2, 4 and 5 that does not read the field: the region, the unclamped source r and the clamped one's cell and
    fraction (x, y, z each), g, wo and the still mask."""
    region, w = weights(rec, N)
    i = np.arange(N, dtype=f32)
    full = lambda v: np.ascontiguousarray(np.broadcast_to(v, (N, N, N)), dtype=f32)
    p = (full(i[:, None, None]), full(i[None, None, :]), full(i[None, :, None]))  # x, y, z
    U = source_coords(list(rec.pull), N)
    last = f32(N - 1)
    with np.errstate(all="ignore"):
        r = [(p[a] + (w * (U[a] - p[a]))).astype(f32) for a in range(3)]
        u = [np.fmin(np.fmax(r[a], f32(0.0)), last) for a in range(3)]
        cell = [np.minimum(np.maximum(np.floor(ua).astype(np.int64), 0), N - 2) for ua in u]
        frac = [(u[a] - cell[a].astype(f32)).astype(f32) for a in range(3)]
        g = (f32(1.0) + (w * (f32(rec.length_scale) - f32(1.0)))).astype(f32)
        off = f32(f32(rec.inflate) * f32(unit))
        wo = (w * off).astype(f32)
        still = (r[0] == p[0]) & (r[1] == p[1]) & (r[2] == p[2]) & (g == f32(1.0)) & (wo == f32(0.0))
    assert all(a.dtype == np.float32 for a in r + frac + [g, wo])
    return {"region": region, "r": r, "cell": cell, "frac": frac, "g": g, "wo": wo, "still": still}


def _result(written, N):
    if not written.any():
        return {"written": 0, "lo": (N, N, N), "hi": (-1, -1, -1)}
    x, z, y = np.nonzero(written)
    return {"written": int(written.sum()), "lo": (int(x.min()), int(y.min()), int(z.min())), "hi": (int(x.max()), int(y.max()), int(z.max()))}


def warp(stored: np.ndarray, material: np.ndarray, fmt: int, rec, extent=None, density_scale: float = 1.0) -> tuple:
    """(stored', material', {"written", "lo", "hi"}, density writes) — lo > hi when nothing was written.  extent: the volume's half size
    (None: a cell of 1)."""
    assert fmt in (F32, TEXEL16) and stored.dtype == np.float32 and material.dtype == np.uint8
    N = stored.shape[0]
    G = geometry(rec, N, units(N, (N - 1) / 2.0 if extent is None else extent, density_scale)[1])
    (cx, cy, cz), (fx, fy, fz) = G["cell"], G["frac"]
    s = decode(stored, fmt)  # step 6: every read sees the volume before the call
    tap = lambda dx, dy, dz: s[cx + dx, cz + dz, cy + dy]
    with np.errstate(all="ignore"):
        c00, c10 = lerp(tap(0, 0, 0), tap(1, 0, 0), fx), lerp(tap(0, 1, 0), tap(1, 1, 0), fx)
        c01, c11 = lerp(tap(0, 0, 1), tap(1, 0, 1), fx), lerp(tap(0, 1, 1), tap(1, 1, 1), fx)
        T = lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz)
        m = ((T * G["g"]) - G["wo"]).astype(f32)
        solid = m <= f32(0.0)
    assert T.dtype == np.float32
    moved = G["region"] & ~G["still"] & (m == m)  # step 5, and never a NaN
    value = texel16_field(m) if fmt == TEXEL16 else m
    if rec.material >= 0:
        ids = np.where(solid, np.uint8(rec.material), np.uint8(0))
    elif rec.material == SOURCE:
        near = lambda c, f: c + (f >= f32(0.5))
        ids = material[near(cx, fx), near(cz, fz), near(cy, fy)]
    else:
        assert rec.material == KEEP
        ids = material
    density = moved & (value.view(np.uint32) != stored.view(np.uint32))
    changed_id = moved & (ids != material)
    out_d, out_m = stored.copy(), material.copy()
    out_d[density] = value[density]
    out_m[changed_id] = ids[changed_id]
    return out_d, out_m, _result(density | changed_id, N), int(density.sum())


def warp_in_place(stored: np.ndarray, material: np.ndarray, fmt: int, rec, extent=None, density_scale: float = 1.0) -> tuple:
    """(stored', material'): the same arithmetic, but sample after sample in storage order, every read seeing what earlier samples have
    already written.  NOT the rule."""
    N = stored.shape[0]
    G = geometry(rec, N, units(N, (N - 1) / 2.0 if extent is None else extent, density_scale)[1])
    (cx, cy, cz), (fx, fy, fz) = G["cell"], G["frac"]
    out_d, out_m = stored.copy(), material.copy()
    scale = f32(0.01) if fmt == TEXEL16 else f32(1.0)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        for x, z, y in zip(*np.nonzero(G["region"] & ~G["still"])):
            i, j, k = cx[x, z, y], cy[x, z, y], cz[x, z, y]
            a, b, c = fx[x, z, y], fy[x, z, y], fz[x, z, y]
            t = out_d[i:i + 2, k:k + 2, j:j + 2] * scale  # [dx, dz, dy]
            l = lambda s0, s1, f: (s0 * (one - f)) + (s1 * f)
            low = l(l(t[0, 0, 0], t[1, 0, 0], a), l(t[0, 0, 1], t[1, 0, 1], a), b)
            high = l(l(t[0, 1, 0], t[1, 1, 0], a), l(t[0, 1, 1], t[1, 1, 1], a), b)
            m = f32((l(low, high, c) * G["g"][x, z, y]) - G["wo"][x, z, y])
            if not m == m:
                continue
            if rec.material >= 0:
                out_m[x, z, y] = rec.material if m <= 0 else 0
            elif rec.material == SOURCE:
                out_m[x, z, y] = out_m[i + (a >= f32(0.5)), k + (c >= f32(0.5)), j + (b >= f32(0.5))]
            out_d[x, z, y] = texel16_field(np.array([m], f32))[0] if fmt == TEXEL16 else m
    return out_d, out_m


# ---- what the rule is worth ---------------------------------------------------------------------------------------------------------

WORTH_N, WORTH_RADIUS, WORTH_REGION, WORTH_FALLOFF = 33, 8.0, 14.0, 2.0


def worth_cases():
    """[(name, fields of the record beyond the region, the moved sphere's centre, its radius)]: the four motions of the header's figures,
    on a sphere of 8 cells about the centre of 33^3 inside a ball region of 14 cells at falloff 2 and strength 1."""
    c = (WORTH_N - 1) / 2.0
    grab = lambda v: tuple(IDENTITY[:3]) + (-v[0],) + tuple(IDENTITY[4:7]) + (-v[1],) + tuple(IDENTITY[8:11]) + (-v[2],)
    k = 1.25
    scale = (1 / k, 0, 0, c - c / k, 0, 1 / k, 0, c - c / k, 0, 0, 1 / k, c - c / k)
    return [("grab by (2.3, -1.1, 0.7)", dict(pull=grab((2.3, -1.1, 0.7))), (c + 2.3, c - 1.1, c + 0.7), WORTH_RADIUS),
            ("grab by (0.5, 0.5, 0.5)", dict(pull=grab((0.5, 0.5, 0.5))), (c + 0.5, c + 0.5, c + 0.5), WORTH_RADIUS),
            ("scale by 1.25", dict(pull=scale, length_scale=k), (c, c, c), WORTH_RADIUS * k),
            ("inflate by 1.5", dict(pull=IDENTITY, inflate=1.5), (c, c, c), WORTH_RADIUS + 1.5)]


def worth(make_record) -> dict:
    """name -> (RMS, mean) of the radial error, in cells, of the warped sphere's zero crossings against the analytic moved sphere.
    make_record(shape, a, b, radius, **fields) builds the record (volumetricraytracer_amd.warp_record)."""
    N, c = WORTH_N, (WORTH_N - 1) / 2.0
    f0 = noisy_sphere(N, WORTH_RADIUS, 0.0)
    ids = np.zeros((N, N, N), np.uint8)
    out = {}
    for name, fields, centre, radius in worth_cases():
        rec = make_record(0, (c, c, c), (0.0, 0.0, 0.0), WORTH_REGION, strength=1.0, falloff=WORTH_FALLOFF, material=KEEP, **fields)
        out[name] = crossing_errors(warp(f0, ids, F32, rec)[0], radius, centre)
    return out
