"""Plain-numpy restatement of the rule of vrt_query_points (include/vrt.h), written from the header rather than from the kernel.

The state is what the device stores: a slot's `stored` is the DENSE buffer [x, z, y] (F32: the densities; TEXEL16: the integer field +-q
as float32) and `material` its ids.  With dtype = np.float32 (the default) every operation is an np.float32 operation in the header's
parenthesisation: numpy's ufuncs round once per operation and never fuse a multiply with an add, and its sqrt and divide are correctly
rounded.  With dtype = np.float64 the same steps run in double on the same fp32 inputs and the same packed fp32 matrices — the yardstick
for placements whose fp32 rounding the header does not pin bit for bit."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

F32, TEXEL16 = 0, 1
SAMPLED = 1
f32 = np.float32


@dataclass
class Slot:
    stored: np.ndarray                 # float32 [x, z, y]
    material: Optional[np.ndarray]     # uint8 [x, z, y] or None
    fmt: int
    extent: float
    density_scale: float = 1.0
    step_max: float = 0.0              # <= 0: unbounded


@dataclass
class Instance:
    slot: int
    position: Sequence[float] = (0.0, 0.0, 0.0)
    rotation: Sequence[float] = (0.0, 0.0, 0.0, 1.0)   # quaternion x, y, z, w
    scale: Sequence[float] = (1.0, 1.0, 1.0)


def pack_w2o(rotation, scale) -> np.ndarray:
    """Step 1's matrix W = R^T S^-1 in fp32, operation by operation: W[i][j] = R[j][i] * (1 / scale[j])."""
    x, y, z, w = (f32(c) for c in rotation)
    one, two = f32(1.0), f32(2.0)
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    R = np.array([[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)],
                  [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
                  [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]], dtype=f32)
    inv_s = np.array([one / f32(s) for s in scale], dtype=f32)
    W = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            W[i, j] = R[j, i] * inv_s[j]
    return W


def smin_of(scale) -> np.float32:
    """Step 2."""
    sx, sy, sz = (np.abs(f32(s)) for s in scale)
    return f32(np.fmin(np.fmin(sx, sy), sz))


def lerp(s0, s1, f, one):
    return (s0 * (one - f)) + (s1 * f)


def evaluate(slots, instances, points, dtype=f32, w2o=None, return_values: bool = False) -> dict:
    """E(p) of every point: a dict of arrays distance, normal, instance, voxel, material, sampled (and, return_values, `values`: every
    instance's value per point, NaN where it contributes nothing, and `h`: step 6's vector before it is normalised).  w2o: the packed fp32 matrices, one per instance (default: pack_w2o)."""
    D = dtype
    zero, one, half = D(0.0), D(1.0), D(0.5)
    p = np.asarray(points, f32).reshape(-1, 3).astype(D)
    n = len(p)
    best = np.full(n, np.inf, D)
    inst = np.full(n, -1, np.int32)
    sampled = np.zeros(n, bool)
    h = np.zeros((n, 3), D)
    voxel = np.full((n, 3), -1, np.int32)
    material = np.zeros(n, np.uint32)
    values = np.full((n, len(instances)), np.nan, np.float64)
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(all="ignore"):
        for k, I in enumerate(instances):
            S = slots[I.slot]
            W = (np.asarray(w2o[k], f32) if w2o is not None else pack_w2o(I.rotation, I.scale)).astype(D)
            pos = np.asarray(I.position, f32).astype(D)
            smin = D(smin_of(I.scale))
            ext = D(f32(S.extent))
            r = p - pos
            q = [(W[a, 0] * r[:, 0] + W[a, 1] * r[:, 1]) + W[a, 2] * r[:, 2] for a in range(3)]            # step 1
            e = [np.abs(qa) - ext for qa in q]                                                          # step 3
            inbox = (e[0] <= zero) & (e[1] <= zero) & (e[2] <= zero)
            m = [np.fmax(ea, zero) for ea in e]
            bound = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) * smin
            N = S.stored.shape[0]                                                                        # step 4
            cell = f32(f32(S.extent) * f32(2.0)) / f32(N - 1)
            inv_cell = D(f32(1.0) / cell)
            g = [(np.where(inbox, qa, zero) + ext) * inv_cell for qa in q]
            c = [np.minimum(np.maximum(np.floor(ga).astype(np.int64), 0), N - 2) for ga in g]
            f = [ga - ca.astype(D) for ga, ca in zip(g, c)]
            stored = np.asarray(S.stored, f32).astype(D)
            s = stored * D(f32(0.01)) if S.fmt == TEXEL16 else stored
            tap = lambda dx, dy, dz: s[c[0] + dx, c[2] + dz, c[1] + dy]
            L = lambda a, b, w: lerp(a, b, w, one)
            s000, s100, s010, s110 = tap(0, 0, 0), tap(1, 0, 0), tap(0, 1, 0), tap(1, 1, 0)
            s001, s101, s011, s111 = tap(0, 0, 1), tap(1, 0, 1), tap(0, 1, 1), tap(1, 1, 1)
            fx, fy, fz = f
            t = L(L(L(s000, s100, fx), L(s010, s110, fx), fy), L(L(s001, s101, fx), L(s011, s111, fx), fy), fz)
            Gx = L(L(s100 - s000, s110 - s010, fy), L(s101 - s001, s111 - s011, fy), fz)
            Gy = L(L(s010 - s000, s110 - s100, fx), L(s011 - s001, s111 - s101, fx), fz)
            Gz = L(L(s001 - s000, s101 - s100, fx), L(s011 - s010, s111 - s110, fx), fy)
            d = t * D(f32(S.density_scale))
            sm = f32(S.step_max)
            if np.isfinite(sm) and sm > 0:
                d = np.fmin(d, D(sm))
            value = np.where(inbox, d * smin, bound)
            contributes = finite & np.where(inbox, ~np.isnan(t), True)
            values[:, k] = np.where(contributes, value, np.nan)
            take = contributes & ((inst < 0) | (value < best))                                           # step 5
            ts = take & inbox
            hk = np.stack([(W[0, a] * Gx + W[1, a] * Gy) + W[2, a] * Gz for a in range(3)], axis=1)      # step 6
            h[ts] = hk[ts]
            near = np.stack([np.minimum(np.maximum(np.floor(ga + half), zero), D(N - 1)).astype(np.int32) for ga in g], axis=1)
            voxel[ts] = near[ts]
            if S.material is not None:
                material[ts] = np.asarray(S.material, np.uint8)[near[:, 0], near[:, 2], near[:, 1]].astype(np.uint32)[ts]
            else:
                material[ts] = 0
            sampled = np.where(take, inbox, sampled)
            best = np.where(take, value, best).astype(D)
            inst = np.where(take, np.int32(k), inst).astype(np.int32)
        H = (h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) + h[:, 2] * h[:, 2]
        ok = sampled & (H != zero) & np.isfinite(H)
        normal = np.where(ok[:, None], h / np.sqrt(H)[:, None], zero).astype(D)
    voxel[~sampled] = -1
    material[~sampled] = 0
    out = {"distance": best, "normal": normal, "instance": inst, "voxel": voxel, "material": material, "sampled": sampled}
    if return_values:
        out["values"], out["h"] = values, h
    return out


def move(position, normal, distance):
    """One projection move in fp32: p_a = p_a - (normal_a * distance)."""
    p, nrm, d = np.asarray(position, f32), np.asarray(normal, f32), np.asarray(distance, f32)
    with np.errstate(all="ignore"):
        return (p - (nrm * d[:, None])).astype(f32)


def goes_on(rec: dict, tolerance: float) -> np.ndarray:
    """Whether a projection moves on from a record: SAMPLED, a normal, and further than the tolerance from the surface."""
    with np.errstate(invalid="ignore"):
        return rec["sampled"] & ~(rec["normal"] == 0).all(axis=1) & ~(np.abs(rec["distance"]) <= f32(tolerance))


def query(slots, instances, points, iterations: int = 0, tolerance: float = 0.0, w2o=None) -> dict:
    """The query of the header, in fp32: the records of evaluate() at the final points, with moves and position."""
    p = np.asarray(points, f32).reshape(-1, 3).copy()
    moves = np.zeros(len(p), np.uint32)
    active = np.ones(len(p), bool)
    for _ in range(iterations):
        rec = evaluate(slots, instances, p, w2o=w2o)
        active = active & goes_on(rec, tolerance)
        if not active.any():
            break
        p[active] = move(p[active], rec["normal"][active], rec["distance"][active])
        moves[active] += 1
    rec = evaluate(slots, instances, p, w2o=w2o)
    rec["moves"], rec["position"] = moves, p
    return rec


def same_bits(got: dict, want: dict) -> list:
    """The fields of two record dicts that differ, floats compared as bits."""
    bad = []
    for key in ("distance", "normal", "position"):
        if not np.array_equal(np.asarray(got[key], f32).view(np.uint32), np.asarray(want[key], f32).view(np.uint32)):
            bad.append(key)
    for key in ("instance", "voxel", "material", "sampled", "moves"):
        if not np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)):
            bad.append(key)
    return bad
