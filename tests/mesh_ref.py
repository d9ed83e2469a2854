"""Plain-numpy reference of vrt_volume_extract_mesh, written from the contract in include/vrt.h rather than from either C++ build: whole
arrays, every operation an np.float32 operation in the header's parenthesisation (numpy's ufuncs round once per operation and never
fuse a multiply with an add; sqrt and division are correctly rounded).  Vertices and quads are found, numbered and ordered with array
operations only (nonzero in storage order, an index volume, one lexsort), so a 129^3 grid takes seconds.

The state is what the device stores, as in the other references: `stored` is the DENSE buffer [x, z, y] (F32: the densities; TEXEL16:
the integer field +-q as float32), `material` the material ids in the same order.  Nothing is written to either."""
from __future__ import annotations

import numpy as np

from volume_ref import F32, TEXEL16

f32 = np.float32


def field(stored: np.ndarray, fmt: int, iso) -> np.ndarray:
    """f [x, z, y]: -0.0f where d is NaN, else fminf(fmaxf(d - iso, -1e18f), 1e18f)."""
    assert fmt in (F32, TEXEL16) and stored.dtype == np.float32
    d = (stored * f32(0.01)).astype(f32) if fmt == TEXEL16 else stored
    with np.errstate(invalid="ignore"):
        f = np.fmin(np.fmax((d - f32(iso)).astype(f32), f32(-1e18)), f32(1e18)).astype(f32)
    f[np.isnan(d)] = f32(-0.0)
    return f


def extract(stored: np.ndarray, material: np.ndarray, fmt: int, iso, extent, lo=None, hi=None):
    """(positions (V, 3) float32 object space, normals (V, 3) float32, materials (V,) uint8, indices (T, 3) uint32, info) of the sample
    box lo..hi (xyz, inclusive; the whole grid without one); info = {"vertices", "quads", "lo", "hi"} as vrt_mesh_result reports."""
    N = stored.shape[0]
    lo = (0, 0, 0) if lo is None else tuple(int(v) for v in lo)
    hi = (N - 1,) * 3 if hi is None else tuple(int(v) for v in hi)
    n = tuple(h - l for l, h in zip(lo, hi))  # cells per axis
    empty = (np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, np.uint8), np.zeros((0, 3), np.uint32),
             {"vertices": 0, "quads": 0, "lo": (N, N, N), "hi": (-1, -1, -1)})
    if min(n) < 1:
        return empty
    F = field(stored, fmt, iso).transpose(0, 2, 1)  # [x, y, z] from here on
    M = material.transpose(0, 2, 1)
    S = F[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    offset = [(j & 1, (j >> 1) & 1, j >> 2) for j in range(8)]
    corner = [S[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]] for dx, dy, dz in offset]
    out = [c > f32(0.0) for c in corner]
    n_out = sum(o.astype(np.int8) for o in out)
    active = (n_out > 0) & (n_out < 8)
    x, z, y = np.nonzero(active.transpose(0, 2, 1))  # the order of the keys (cx * N + cz) * N + cy
    V = x.size
    if V == 0:
        return empty
    rel = (x, y, z)
    c = [rel[a] + lo[a] for a in range(3)]
    fv = [cj[x, y, z] for cj in corner]
    ov = [oj[x, y, z] for oj in out]

    g = [np.zeros(V, f32) for _ in range(3)]
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
                    g[a] = (g[a] + (fb - fa)).astype(f32)
                    cross = ov[A] != ov[B]
                    t = (fa / (fa - fb)).astype(f32)
                    s[a] = np.where(cross, s[a] + t, s[a]).astype(f32)
                    s[b] = np.where(cross, s[b] + f32(ob), s[b]).astype(f32)
                    s[cc] = np.where(cross, s[cc] + f32(oc), s[cc]).astype(f32)
                    k += cross
        cell = (f32(extent) * f32(2.0)) / f32(N - 1)
        kf = k.astype(f32)
        p = [(c[a].astype(f32) + (s[a] / kf)).astype(f32) for a in range(3)]
        positions = np.stack([((p[a] * cell) - f32(extent)).astype(f32) for a in range(3)], axis=1)
        G = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(f32)
        root = np.sqrt(G).astype(f32)
        normals = np.stack([np.where(G == f32(0.0), f32(0.0), g[a] / root).astype(f32) for a in range(3)], axis=1)

    inside = np.stack([~o for o in ov], axis=1)
    first = np.argmax(inside, axis=1)  # the lowest-numbered INSIDE corner
    off = np.array(offset)[first]
    materials = np.ascontiguousarray(M[c[0] + off[:, 0], c[1] + off[:, 1], c[2] + off[:, 2]], dtype=np.uint8)

    number = np.full(n, -1, np.int64)
    number[x, y, z] = np.arange(V)
    quads, keys, axes = [], [], []
    for a in range(3):
        b, cc = (a + 1) % 3, (a + 2) % 3
        differ = out[0] != out[1 << a]  # sample A is corner 0 of the cell with its index, B = A + 1 on a is corner 1 << a
        ok = np.zeros(n, bool)
        inner = [slice(None)] * 3
        inner[b], inner[cc] = slice(1, None), slice(1, None)  # the cells one index below on b and c lie in the cell box
        ok[tuple(inner)] = differ[tuple(inner)]
        at = list(np.nonzero(ok))
        a_out = out[0][tuple(at)]
        q = []
        for db, dc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            w = list(at)
            w[b], w[cc] = at[b] + db, at[cc] + dc
            q.append(number[tuple(w)])
        q = np.stack(q, axis=1)
        assert (q >= 0).all()  # all four are active by construction
        quads.append(np.where(a_out[:, None], q[:, ::-1], q))
        keys.append(((at[0] + lo[0]) * N + (at[2] + lo[2])) * N + (at[1] + lo[1]))
        axes.append(np.full(at[0].size, a))
    quads, keys, axes = np.concatenate(quads), np.concatenate(keys), np.concatenate(axes)
    quads = quads[np.lexsort((axes, keys))]
    indices = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.uint32)
    info = {"vertices": int(V), "quads": int(quads.shape[0]), "lo": tuple(int(v.min()) for v in c), "hi": tuple(int(v.max()) for v in c)}
    return positions, normals, materials, indices, info


# ---- properties of a mesh ----------------------------------------------------------------------------------------------------------

def directed_edges(indices: np.ndarray) -> np.ndarray:
    """(3 T, 2) int64: every triangle's edges in its own direction."""
    t = indices.astype(np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_census(indices: np.ndarray, n_vertices: int):
    """(most often a directed edge occurs, the directed edges without their reverse (K, 2), undirected edge count)."""
    e = directed_edges(indices)
    code = e[:, 0] * n_vertices + e[:, 1]
    uniq, count = np.unique(code, return_counts=True)
    reverse = (uniq % n_vertices) * n_vertices + uniq // n_vertices
    unpaired = uniq[~np.isin(reverse, uniq)]
    undirected = np.unique(np.minimum(e[:, 0], e[:, 1]) * n_vertices + np.maximum(e[:, 0], e[:, 1])).size
    return int(count.max()) if count.size else 0, np.stack([unpaired // n_vertices, unpaired % n_vertices], axis=1), int(undirected)


def triangle_normals(positions: np.ndarray, indices: np.ndarray) -> np.ndarray:
    p = positions.astype(np.float64)
    p0, p1, p2 = (p[indices[:, i].astype(np.int64)] for i in range(3))
    return np.cross(p1 - p0, p2 - p0)


def signed_volume(positions: np.ndarray, indices: np.ndarray) -> float:
    p = positions.astype(np.float64)
    p0, p1, p2 = (p[indices[:, i].astype(np.int64)] for i in range(3))
    return float(np.einsum("ij,ij->i", p0, np.cross(p1, p2)).sum() / 6.0)
