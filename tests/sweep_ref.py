"""Plain-numpy restatement of the rule of vrt_query_sweeps (include/vrt.h), written from the header rather than from the kernel.

The per-instance steps are points_ref's: every evaluation of instance k goes through points_ref.evaluate(slots, [I], p).  With
dtype = np.float32 (the default) every operation here is an np.float32 operation in the header's parenthesisation; with np.float64 the
same steps run in double on the same fp32 inputs (the centre p is handed to points_ref as fp32, as every point is) — the yardstick for
placements whose fp32 rounding the header does not pin.  `margin`: the run also marks the records that the header's comparisons decide
by less than it (see `sweep`)."""
from __future__ import annotations

import numpy as np

import points_ref as P

HIT, EXHAUSTED, INITIAL = 1, 2, 4
f32 = np.float32


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def reach(slots, I, D=f32):
    """Step 2's Rb, in fp32 whatever D is: the library computes it once, on the host, and hands the kernel the fp32 number."""
    sx, sy, sz = (np.abs(f32(s)) for s in I.scale)
    smax = f32(np.fmax(np.fmax(sx, sy), sz))
    ext = f32(slots[I.slot].extent)
    return D(f32(np.sqrt(f32(f32(f32(3.0) * ext) * ext)) * smax))


def bad_records(o, d, t_max, radius):
    """Step 0, on the fp32 inputs."""
    with np.errstate(all="ignore"):
        L = dot(d, d)
        bad = ~np.isfinite(o).all(axis=1) | ~np.isfinite(d).all(axis=1) | (L == 0) | ~np.isfinite(L)
        bad |= ~(t_max >= 0) | ~np.isfinite(t_max) | ~(radius >= 0) | ~np.isfinite(radius)
    return bad


def candidates(slots, instances, o, u, t_max, radius, D=f32, margin=None):
    """Step 2: [n, n_inst] bools; with a margin, also the records where a test is decided by less than 1e-4 relative."""
    n = len(o)
    cand = np.zeros((n, len(instances)), bool)
    close = np.zeros(n, bool)
    zero = D(0.0)
    with np.errstate(all="ignore"):
        for k, I in enumerate(instances):
            m = np.asarray(I.position, f32).astype(D)[None, :] - o
            s = np.fmin(np.fmax(dot(m, u), zero), t_max)
            e = m - (u * s[:, None])
            B = (reach(slots, I, D) + radius) * D(f32(1.0001))
            ee, BB = dot(e, e), B * B
            cand[:, k] = ee <= BB
            if margin is not None:
                close |= np.abs(ee - BB) <= 1e-4 * BB
    return cand, close


def sweep(slots, instances, sweeps, max_steps, tolerance, step_min, dtype=f32, w2o=None, margin=None) -> dict:
    """The query of the header: a dict of arrays t, normal, instance, voxel, material, flags, steps, distance, position (and `cand`, the
    candidates of step 2).  sweeps: a structured array with origin, t_max, direction, radius (renderer.SWEEP_DTYPE).  margin (world
    units): adds `ambiguous` — the records for which, at some step, the hit decision c <= tolerance, the choice between the two
    smallest clearances, a box face (the margin over smin, in object space) or t <= t_max lies within the margin, whose candidate test
    lies within 1e-4 relative, or whose step count reached max_steps."""
    D = dtype
    o32, d32 = np.asarray(sweeps["origin"], f32), np.asarray(sweeps["direction"], f32)
    tm32, r32 = np.asarray(sweeps["t_max"], f32), np.asarray(sweeps["radius"], f32)
    n = len(o32)
    bad = bad_records(o32, d32, tm32, r32)
    o, d, t_max, radius = o32.astype(D), d32.astype(D), tm32.astype(D), r32.astype(D)
    tol, smin_step = D(f32(tolerance)), D(f32(step_min))
    with np.errstate(all="ignore"):
        L = dot(d, d)
        inv = D(1.0) / np.sqrt(L)
        u = d * inv[:, None]
        cand, amb = candidates(slots, instances, o, u, t_max, radius, D, margin)
    cand[bad] = False
    amb &= ~bad
    t = np.zeros(n, D)
    steps = np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint32)
    position = o.copy()
    out_t = np.full(n, -1.0, D)
    normal = np.zeros((n, 3), D)
    instance = np.full(n, -1, np.int32)
    voxel = np.full((n, 3), -1, np.int32)
    material = np.zeros(n, np.uint32)
    distance = np.full(n, np.inf, D)
    active = ~bad
    with np.errstate(all="ignore"):
        while active.any():
            ia = np.flatnonzero(active)
            p = o[ia] + (u[ia] * t[ia][:, None])
            position[ia] = p
            past = t[ia] > t_max[ia]
            if margin is not None:
                amb[ia] |= np.abs(t[ia] - t_max[ia]) <= margin
            out_of_steps = ~past & (steps[ia] == max_steps)
            flags[ia[out_of_steps]] = EXHAUSTED
            out_t[ia[out_of_steps]] = t[ia[out_of_steps]]
            go = ~past & ~out_of_steps
            active[ia[~go]] = False
            ia, p = ia[go], p[go]
            if len(ia) == 0:
                break
            steps[ia] += 1
            m = len(ia)
            best_c = np.full(m, np.inf, D)
            cs = np.full((m, len(instances)), np.inf, np.float64)  # (margin) the clearances of the distinct contributors
            best_k = np.full(m, -1, np.int32)
            best_s = np.zeros(m, bool)
            rec = {"distance": np.full(m, np.inf, D), "normal": np.zeros((m, 3), D), "voxel": np.full((m, 3), -1, np.int32),
                   "material": np.zeros(m, np.uint32)}
            p32 = p.astype(f32)
            for k, I in enumerate(instances):
                sub = np.flatnonzero(cand[ia, k])
                if len(sub) == 0:
                    continue
                one = P.evaluate(slots, [I], p32[sub], dtype=D, w2o=None if w2o is None else [w2o[k]])
                contributes = one["instance"] == 0
                c = np.where(one["sampled"], one["distance"] - radius[ia[sub]], one["distance"])
                take = contributes & ((best_k[sub] < 0) | (c < best_c[sub]))
                if margin is not None:
                    placements = (I.slot, tuple(I.position), tuple(I.rotation), tuple(I.scale))
                    twin = any(placements == (J.slot, tuple(J.position), tuple(J.rotation), tuple(J.scale)) for J in instances[:k])
                    if not twin:  # an exact duplicate computes the same bits: no doubt there
                        cs[sub, k] = np.where(contributes, c, np.inf)
                    W = (P.pack_w2o(I.rotation, I.scale) if w2o is None else np.asarray(w2o[k], f32)).astype(np.float64)
                    q = (p[sub].astype(np.float64) - np.asarray(I.position, f32).astype(np.float64)) @ W.T
                    ext = float(f32(slots[I.slot].extent))
                    amb[ia[sub]] |= (np.abs(np.abs(q) - ext) <= margin / float(P.smin_of(I.scale))).any(axis=1)
                ts = sub[take]
                best_c[ts], best_k[ts], best_s[ts] = c[take], k, one["sampled"][take]
                for key in rec:
                    rec[key][ts] = one[key][take]
            if margin is not None:
                cs.sort(axis=1)
                if cs.shape[1] > 1:
                    amb[ia] |= (cs[:, 1] - cs[:, 0]) <= margin
                amb[ia] |= best_s & (np.abs(best_c.astype(np.float64) - float(tol)) <= margin)
            nothing = best_k < 0
            hit = ~nothing & best_s & (best_c <= tol)
            ih = ia[hit]
            flags[ih] = HIT | np.where(steps[ih] == 1, INITIAL, 0).astype(np.uint32)
            out_t[ih], instance[ih] = t[ih], best_k[hit]
            for key, dst in (("distance", distance), ("normal", normal), ("voxel", voxel), ("material", material)):
                dst[ih] = rec[key][hit]
            active[ia[nothing | hit]] = False
            on = ~(nothing | hit)
            t[ia[on]] = t[ia[on]] + np.fmax(best_c[on], smin_step)
    out = {"t": out_t, "normal": normal, "instance": instance, "voxel": voxel, "material": material, "flags": flags, "steps": steps,
           "distance": distance, "position": position, "cand": cand}
    if margin is not None:
        out["ambiguous"] = amb | (steps >= max_steps)
    return out


FLOATS, INTS = ("t", "normal", "distance", "position"), ("instance", "voxel", "material", "flags", "steps")


def same_bits(got: dict, want: dict) -> list:
    """The fields of two record dicts that differ, floats compared as bits."""
    bad = []
    for key in FLOATS:
        if not np.array_equal(np.asarray(got[key], f32).view(np.uint32), np.asarray(want[key], f32).view(np.uint32)):
            bad.append(key)
    for key in INTS:
        if not np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)):
            bad.append(key)
    return bad


def chain(evaluate_one, reach_ok, sweeps, max_steps, tolerance, step_min) -> dict:
    """Consequence (b): a sweep of a one-instance scene as its evaluations chained through a plain point query.  evaluate_one(points)
    -> a record dict of vrt_query_points (iterations 0); reach_ok: [n] bools, whether the instance is a candidate of the record.
    All of it in fp32."""
    o, d = np.asarray(sweeps["origin"], f32), np.asarray(sweeps["direction"], f32)
    t_max, radius = np.asarray(sweeps["t_max"], f32), np.asarray(sweeps["radius"], f32)
    n = len(o)
    bad = bad_records(o, d, t_max, radius)
    with np.errstate(all="ignore"):
        L = dot(d, d)
        u = (d * (f32(1.0) / np.sqrt(L))[:, None]).astype(f32)
    t = np.zeros(n, f32)
    steps = np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint32)
    out = {"t": np.full(n, -1.0, f32), "normal": np.zeros((n, 3), f32), "instance": np.full(n, -1, np.int32),
           "voxel": np.full((n, 3), -1, np.int32), "material": np.zeros(n, np.uint32), "distance": np.full(n, np.inf, f32)}
    position = o.copy()
    active = ~bad
    with np.errstate(all="ignore"):
        while active.any():
            ia = np.flatnonzero(active)
            p = (o[ia] + (u[ia] * t[ia][:, None])).astype(f32)
            position[ia] = p
            past = t[ia] > t_max[ia]
            spent = ~past & (steps[ia] == max_steps)
            flags[ia[spent]] = EXHAUSTED
            out["t"][ia[spent]] = t[ia[spent]]
            go = ~past & ~spent
            active[ia[~go]] = False
            ia, p = ia[go], p[go]
            if len(ia) == 0:
                break
            steps[ia] += 1
            one = evaluate_one(p)
            contributes = (one["instance"] == 0) & reach_ok[ia]
            c = np.where(one["sampled"], one["distance"] - radius[ia], one["distance"]).astype(f32)
            hit = contributes & one["sampled"] & (c <= f32(tolerance))
            ih = ia[hit]
            flags[ih] = HIT | np.where(steps[ih] == 1, INITIAL, 0).astype(np.uint32)
            out["t"][ih] = t[ih]
            for key in ("normal", "instance", "voxel", "material", "distance"):
                out[key][ih] = one[key][hit]
            active[ia[~contributes | hit]] = False
            on = contributes & ~hit
            t[ia[on]] = t[ia[on]] + np.fmax(c[on], f32(step_min))
    out.update(flags=flags, steps=steps, position=position)
    return out
