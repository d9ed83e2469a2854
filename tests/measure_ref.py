"""Plain-numpy reference of vrt_volume_measure, written from the contract in include/vrt.h rather than from either C++ build: whole
arrays, fp32 where the rule is fp32 (numpy's ufuncs round once per operation and never fuse a multiply with an add; sqrt is correctly
rounded), integers for everything that is summed (int64 arrays, whose range the header's derivation covers; the results leave as
Python ints).  The sub-samples are laid out as one boolean volume of 4 x 4 x 4 per cell, and the
sums are taken over its planes and pairs of axes — no closed form for full cells, no per-cell loop.  The quads, their order and their
vertex numbers come from mesh_ref.extract; the vertices' grid coordinates (rule 3 of the mesh, which extract only returns in object
space) are restated here.  properties() restates rule 7 in float64.

The state is what the device stores, as in the other references: `stored` is the DENSE buffer [x, z, y], `material` the material ids in
the same order.  Nothing is written to either."""
from __future__ import annotations

import numpy as np

import mesh_ref as MR

f32 = np.float32
SUB = 4
FIELDS = ("lo", "hi", "subsamples", "moment1", "moment2", "solid_samples", "active_cells", "crossings", "quads", "area_q", "material_samples")


def _lerp(s0, s1, u):
    return ((s0 * (f32(1.0) - u)).astype(f32) + (s1 * u).astype(f32)).astype(f32)


def _trilinear(f, ux, uy, uz):
    c00, c10, c01, c11 = _lerp(f[0], f[1], ux), _lerp(f[2], f[3], ux), _lerp(f[4], f[5], ux), _lerp(f[6], f[7], ux)
    return _lerp(_lerp(c00, c10, uy), _lerp(c01, c11, uy), uz)


def grid_vertices(fv, ov, c):
    """Rule 3 of vrt_volume_extract_mesh for the active cells c (three int arrays) with corner values fv[j] and classes ov[j]: the
    vertices' grid coordinates p_a = (float)c_a + (s_a / (float)k), three float32 arrays."""
    V = c[0].size
    s = [np.zeros(V, f32) for _ in range(3)]
    k = np.zeros(V, np.int32)
    with np.errstate(all="ignore"):
        for a in range(3):
            b, cc = (a + 1) % 3, (a + 2) % 3
            for ob in (0, 1):
                for oc in (0, 1):
                    A = (ob << b) | (oc << cc)
                    B = A | (1 << a)
                    fa, fb = fv[A], fv[B]
                    cross = ov[A] != ov[B]
                    t = (fa / (fa - fb)).astype(f32)
                    s[a] = np.where(cross, s[a] + t, s[a]).astype(f32)
                    s[b] = np.where(cross, s[b] + f32(ob), s[b]).astype(f32)
                    s[cc] = np.where(cross, s[cc] + f32(oc), s[cc]).astype(f32)
                    k += cross
        return [(c[a].astype(f32) + (s[a] / k.astype(f32))).astype(f32) for a in range(3)]


def _cross_len(u, w):
    x = ((u[1] * w[2]).astype(f32) - (u[2] * w[1]).astype(f32)).astype(f32)
    y = ((u[2] * w[0]).astype(f32) - (u[0] * w[2]).astype(f32)).astype(f32)
    z = ((u[0] * w[1]).astype(f32) - (u[1] * w[0]).astype(f32)).astype(f32)
    return np.sqrt((((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32)).astype(f32)).astype(f32)


def quad_areas(p, quads):
    """A per quad (float32), rule 6: p the vertices' grid coordinates (three arrays), quads (Q, 4) vertex numbers v0..v3."""
    v = [[p[a][quads[:, i]] for a in range(3)] for i in range(4)]
    e1, e2, e3 = ([(v[i][a] - v[0][a]).astype(f32) for a in range(3)] for i in (1, 2, 3))
    return ((f32(0.5) * _cross_len(e1, e2)).astype(f32) + (f32(0.5) * _cross_len(e2, e3)).astype(f32)).astype(f32)


def measure(stored: np.ndarray, material: np.ndarray, fmt: int, iso, lo=None, hi=None) -> dict:
    """vrt_measure_result's fields and "material_samples" (256 counts) of the sample box lo..hi (xyz, inclusive; the whole grid
    without one), as Python ints and tuples of them."""
    N = stored.shape[0]
    lo = (0, 0, 0) if lo is None else tuple(int(v) for v in lo)
    hi = (N - 1,) * 3 if hi is None else tuple(int(v) for v in hi)
    n = tuple(h - l for l, h in zip(lo, hi))  # cells per axis
    F = MR.field(stored, fmt, iso).transpose(0, 2, 1)  # [x, y, z] from here on
    M = material.transpose(0, 2, 1)
    box = tuple(slice(l, h + 1) for l, h in zip(lo, hi))
    S = F[box]
    outside = S > f32(0.0)
    out = {"solid_samples": int((~outside).sum()),
           "material_samples": tuple(int(v) for v in np.bincount(M[box][~outside].astype(np.int64), minlength=256)),
           "crossings": tuple(int((np.diff(outside.astype(np.int8), axis=a) != 0).sum()) for a in range(3)),
           "lo": (N, N, N), "hi": (-1, -1, -1), "subsamples": 0, "moment1": (0, 0, 0), "moment2": (0,) * 6, "active_cells": 0, "quads": 0,
           "area_q": 0}
    if min(n) < 1:
        return out
    offset = [(j & 1, (j >> 1) & 1, j >> 2) for j in range(8)]
    corner = [S[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]] for dx, dy, dz in offset]
    cls = [c > f32(0.0) for c in corner]
    n_out = sum(o.astype(np.int8) for o in cls)
    active = (n_out > 0) & (n_out < 8)
    # rules 3 and 4: the sub-samples as a volume of 4 per cell and axis; sub-sample k of an axis sits at X = 8 lo + 2 k + 1
    inside = np.repeat(np.repeat(np.repeat(n_out == 0, SUB, 0), SUB, 1), SUB, 2)
    x, z, y = np.nonzero(active.transpose(0, 2, 1))  # the order of the mesh's vertices
    fv = [cj[x, y, z] for cj in corner]
    u = [f32(0.125) + f32(0.25) * f32(i) for i in range(SUB)]
    for ix in range(SUB):
        for iy in range(SUB):
            for iz in range(SUB):
                t = _trilinear(fv, u[ix], u[iy], u[iz])
                inside[SUB * x + ix, SUB * y + iy, SUB * z + iz] = ~(t > f32(0.0))
    # int64 holds every sum (S2 < 2^57 at N = 513, the header's derivation); the results leave as Python ints
    X = [8 * lo[a] + 2 * np.arange(SUB * n[a], dtype=np.int64) + 1 for a in range(3)]
    plane = [inside.sum(axis=tuple(b for b in range(3) if b != a), dtype=np.int64) for a in range(3)]
    mixed = lambda a, b: int((np.outer(X[a], X[b]) * inside.sum(axis=3 - a - b, dtype=np.int64)).sum())
    out["subsamples"] = int(inside.sum(dtype=np.int64))
    out["moment1"] = tuple(int((X[a] * plane[a]).sum()) for a in range(3))
    out["moment2"] = tuple(int((X[a] * X[a] * plane[a]).sum()) for a in range(3)) + (mixed(0, 1), mixed(0, 2), mixed(1, 2))
    cells = inside.reshape(n[0], SUB, n[1], SUB, n[2], SUB).any(axis=(1, 3, 5))
    if cells.any():
        at = np.nonzero(cells)
        out["lo"] = tuple(int(at[a].min()) + lo[a] for a in range(3))
        out["hi"] = tuple(int(at[a].max()) + lo[a] for a in range(3))
    # rule 6: the mesh's quads with the vertices in grid coordinates
    out["active_cells"] = int(x.size)
    if x.size:
        indices, info = MR.extract(stored, material, fmt, iso, 1.0, lo, hi)[3:]
        assert info["vertices"] == x.size
        quads = np.concatenate([indices[0::2].astype(np.int64), indices[1::2, 2:3].astype(np.int64)], axis=1)  # (v0, v1, v2) + v3 of (v0, v2, v3)
        p = grid_vertices(fv, [cj[x, y, z] for cj in cls], [x + lo[0], y + lo[1], z + lo[2]])
        A = quad_areas(p, quads)
        out["quads"] = int(quads.shape[0])
        out["area_q"] = sum(int(v) for v in np.floor((A * f32(65536.0)).astype(f32) + f32(0.5)).astype(f32))
    return out


def properties(m: dict, N: int, extent) -> dict:
    """Rule 7 in float64."""
    cell = float(f32(f32(extent) * f32(2.0)) / f32(N - 1))
    h, e = cell / 8.0, float(f32(extent))
    out = {"volume": 0.0, "area": 0.0, "centroid": (0.0,) * 3, "inertia": (0.0,) * 6,
           "box_lo": tuple(m["lo"][a] * cell - e for a in range(3)), "box_hi": tuple((m["hi"][a] + 1) * cell - e for a in range(3))}
    S0 = float(m["subsamples"])
    if m["subsamples"] == 0:
        return out
    S1 = [float(v) for v in m["moment1"]]
    s = 2.0 * h  # a sub-sample stands for a cube of side cell / 4
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    Cm = [(float(m["moment2"][i]) - S1[a] * S1[b] / S0) * (h ** 2 * s ** 3) + (S0 * (s ** 5 / 12.0) if a == b else 0.0)
          for i, (a, b) in enumerate(pairs)]
    tr = Cm[0] + Cm[1] + Cm[2]
    out.update(volume=S0 * s ** 3, area=m["area_q"] / 65536.0 * cell * cell, centroid=tuple(S1[a] / S0 * h - e for a in range(3)),
               inertia=tuple((tr if i < 3 else 0.0) - Cm[i] for i in range(6)))
    return out
