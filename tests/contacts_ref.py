"""Plain-numpy restatement of the rule of vrt_query_contacts (include/vrt.h), written from the header rather than from either C++ build.
It composes the two references the rule itself is composed of — mesh_ref.extract (the mesh rule's steps 1 to 3: A's vertices, their
normals and materials) and points_ref.evaluate (the points rule for a scene that holds B alone) — and adds step 2, the object-to-world
transform, as np.float32 operations in the header's parenthesisation.

The state is what the device stores, as in those references: a points_ref.Slot per side (`stored` the DENSE buffer [x, z, y], `material`
its ids) and a points_ref.Instance per placement."""
from __future__ import annotations

import numpy as np

import mesh_ref as M
import points_ref as P

f32 = np.float32
FLOATS = ("position", "distance", "normal", "normal_a")
INTS = ("material_a", "material_b", "cell_a")
SCALARS = ("lo", "hi", "contacts", "candidates")


def pack_o2w(rotation, scale) -> np.ndarray:
    """Step 2's matrix O = S R in fp32, operation by operation: O[i][j] = scale[i] * R[i][j], R as points_ref.pack_w2o builds it."""
    x, y, z, w = (f32(c) for c in rotation)
    one, two = f32(1.0), f32(2.0)
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    R = np.array([[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)],
                  [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
                  [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]], dtype=f32)
    O = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            O[i, j] = f32(scale[i]) * R[i, j]
    return O


def active_cells(stored: np.ndarray, fmt: int) -> np.ndarray:
    """The active cells of the whole grid at iso 0, (V, 3) xyz, in the order of their keys (cx*N + cz)*N + cy: mesh_ref.extract's order."""
    N = stored.shape[0]
    F = M.field(np.asarray(stored, f32), fmt, 0.0).transpose(0, 2, 1)  # [x, y, z]
    n = N - 1
    n_out = sum((F[dx:dx + n, dy:dy + n, dz:dz + n] > f32(0.0)).astype(np.int8) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    x, z, y = np.nonzero(((n_out > 0) & (n_out < 8)).transpose(0, 2, 1))
    return np.stack([x, y, z], axis=1).astype(np.int32)


def distance_key(d: np.ndarray) -> np.ndarray:
    """Step 5's order of distances: fp32 onto unsigned, order-preserving, -0 below +0."""
    u = np.asarray(d, f32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def world_points(slot_a: P.Slot, inst_a: P.Instance):
    """Steps 1 and 2: (cells (V, 3), world points (V, 3) float32, vertex normals (V, 3) float32, materials (V,)) of A's surface."""
    material = slot_a.material if slot_a.material is not None else np.zeros(slot_a.stored.shape, np.uint8)
    positions, normals, materials, _, info = M.extract(np.asarray(slot_a.stored, f32), np.asarray(material, np.uint8), slot_a.fmt, 0.0, slot_a.extent)
    cells = active_cells(slot_a.stored, slot_a.fmt)
    assert len(cells) == info["vertices"] == len(positions)
    O = pack_o2w(inst_a.rotation, inst_a.scale)
    pos = np.asarray(inst_a.position, f32)
    o = positions.astype(f32)
    with np.errstate(all="ignore"):
        w = np.stack([(((O[a, 0] * o[:, 0] + O[a, 1] * o[:, 1]).astype(f32) + O[a, 2] * o[:, 2]).astype(f32) + pos[a]).astype(f32) for a in range(3)],
                     axis=1)
    return cells, w, normals, materials


def contacts(slot_a: P.Slot, inst_a: P.Instance, slot_b: P.Slot, inst_b: P.Instance, margin: float = 0.0) -> dict:
    """The records and the result of vrt_query_contacts(a, b, margin): arrays position, distance, normal, material_a, normal_a,
    material_b, cell_a in the contacts' order, and lo, hi, contacts, candidates, min_distance."""
    N = slot_a.stored.shape[0]
    cells, w, n_a, mat_a = world_points(slot_a, inst_a)
    rec = P.evaluate([slot_b], [P.Instance(0, inst_b.position, inst_b.rotation, inst_b.scale)], w)  # steps 3: B alone
    candidate = rec["sampled"]
    with np.errstate(invalid="ignore"):
        hit = candidate & (rec["distance"] <= f32(margin))
    W = P.pack_w2o(inst_a.rotation, inst_a.scale)
    n = n_a[hit].astype(f32)
    with np.errstate(all="ignore"):
        h = np.stack([((W[0, a] * n[:, 0] + W[1, a] * n[:, 1]).astype(f32) + W[2, a] * n[:, 2]).astype(f32) for a in range(3)], axis=1)
        H = ((h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]).astype(f32) + h[:, 2] * h[:, 2]).astype(f32)
        ok = (H != f32(0.0)) & np.isfinite(H)
        normal_a = np.where(ok[:, None], h / np.sqrt(H)[:, None], f32(0.0)).astype(f32)
    out = {"position": w[hit], "distance": rec["distance"][hit].astype(f32), "normal": rec["normal"][hit].astype(f32),
           "material_a": mat_a[hit].astype(np.uint32), "normal_a": normal_a, "material_b": rec["material"][hit].astype(np.uint32),
           "cell_a": cells[hit], "contacts": int(hit.sum()), "candidates": int(candidate.sum())}
    if hit.any():
        out["lo"], out["hi"] = tuple(int(v) for v in cells[hit].min(axis=0)), tuple(int(v) for v in cells[hit].max(axis=0))
        d = out["distance"]
        out["min_distance"] = float(d[np.argmin(distance_key(d))])
    else:
        out["lo"], out["hi"], out["min_distance"] = (N, N, N), (-1, -1, -1), float("inf")
    return out


def same_bits(got: dict, want: dict) -> list:
    """The fields of two contact dicts that differ, floats compared as bits."""
    bad = []
    for key in FLOATS:
        a, b = np.asarray(got[key], f32), np.asarray(want[key], f32)
        if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            bad.append(key)
    for key in INTS:
        a, b = np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)
        if a.shape != b.shape or not np.array_equal(a, b):
            bad.append(key)
    for key in SCALARS:
        if tuple(np.atleast_1d(got[key]).tolist()) != tuple(np.atleast_1d(want[key]).tolist()):
            bad.append(key)
    if f32(got["min_distance"]).view(np.uint32) != f32(want["min_distance"]).view(np.uint32):
        bad.append("min_distance")
    return bad
