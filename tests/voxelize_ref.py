"""Independent float64 reference of vrt_voxelize_mesh and of the CPU converter, restated from the sentence in include/vrt.h —
"density = dist/thr - 0.5 (thr = cell*sqrt 3) in every triangle's (bbox +- thr +- 1 voxel) index box, minimum over triangles,
background 2*extent, material = (density <= 0)" — and from nothing in csrc/voxelize_core.h: the distance comes from Ericson's
closest point, which shares nothing with the converter's 7-region classification, and the box from min / max of the vertices.

The rule.  N = 2^resolution + 1; cell = 2*extent/(N-1) and thr = cell*sqrt(3) are the fp32 values the API computes (inputs of the
contract, not results); voxel i sits at i*cell - extent.  On each axis a triangle's box is
round((min - thr + extent)/cell) - 1 ... round((max + thr + extent)/cell) + 1, clipped to 0 ... N-1, round = half away from zero.
A voxel's density starts at 2*extent and becomes the minimum with dist/thr - 0.5 over the triangles whose box holds it (the
background takes part in the minimum); material = 1 where density <= 0.  Arrays are indexed [x, z, y] like a downloaded volume.
A triangle is skipped, and counted, when one of its indices is out of range, one of its vertices holds a NaN, or its area or one
of its edges is zero; 1-2 trailing indices are ignored.

Ambiguity.  fp32 and float64 may round a box edge to different voxels when the value before rounding lies next to a tie (x.5).
reference() counts the edges within AMBIGUOUS = 1e-3 voxels of a tie whose two roundings give different clipped indices; every
case builder redraws until that count is 0 and every test asserts it.  (The fp32 value differs from the float64 one by a few ulps
of a number <= 513 plus a few ulps of a coordinate over cell: below 3e-4 voxels at resolution 9, less elsewhere.)

Tolerance.  A density is a distance built from coordinate differences of magnitude <= extent, divided by
thr = 2*extent*sqrt(3)/(N-1): an error of k ulps (2^-23 relative) of such a coordinate costs k * (N-1)/(2 sqrt 3) * 2^-23 in density.
Voxel position (one product, one sum), the three differences, the dot products with unit vectors that are themselves rounded and
the final division allow k ~ 14 ulps: tol = 4 * (N-1) * 2^-23 * max(1, |want|), the factor 4 being 14/(2 sqrt 3) rounded.  It is
derived, not tuned, and holds for WELL-CONDITIONED triangles only: smallest angle >= 15 degrees, shortest edge >= cell/4 (the unit
vectors of a needle or of a sub-cell triangle carry a relative error that is not bounded by ulps of extent).
profiles/voxelize_reference.txt lists the worst scaled error measured per case, in units of (N-1) * 2^-23."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

EXTENT = 50.0
AMBIGUOUS = 1e-3
MIN_ANGLE_DEG = 15.0
LEFT_OUT_SHARE = 1e-3  # of a case's voxels, at most, may lie within tol of density 0 and so go without a material check


def grid(resolution: int, extent: float):
    """(N, cell, thr): cell and thr as the fp32 values vrt_voxelize_mesh computes, returned as Python floats."""
    N = (1 << resolution) + 1
    cell = np.float32(np.float32(extent) * np.float32(2.0)) / np.float32(N - 1)
    thr = np.float32(cell * np.sqrt(np.float32(3.0)))
    return N, float(cell), float(thr)


def tol(N: int, want):
    return 4.0 * (N - 1) * 2.0 ** -23 * np.maximum(1.0, np.abs(want))


def scaled_error(N: int, got, want) -> float:
    """Worst |got - want| / max(1, |want|) in units of (N-1) * 2^-23: the tolerance is 4 of them."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max() / ((N - 1) * 2.0 ** -23))


def point_triangle_distance(P, A, B, C):
    """Closest-point-on-triangle distance (Ericson, Real-Time Collision Detection 5.1.5), float64, vectorised over points —
    an algorithm that shares nothing with the Voxelizer's 7-region classification."""
    ab, ac, ap = B - A, C - A, P - A
    d1, d2 = ap @ ab, ap @ ac
    bp = P - B
    d3, d4 = bp @ ab, bp @ ac
    cp = P - C
    d5, d6 = cp @ ab, cp @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    out = np.empty(len(P))
    with np.errstate(divide="ignore", invalid="ignore"):
        vq = d1 / (d1 - d3)
        wq = d2 / (d2 - d6)
        wr = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    closest = A + np.outer(vb * den, ab) + np.outer(vc * den, ac)  # interior
    m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    closest[m] = B + np.outer(wr, C - B)[m]
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    closest[m] = A + np.outer(wq, ac)[m]
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    closest[m] = A + np.outer(vq, ab)[m]
    closest[(d6 >= 0) & (d5 <= d6)] = C
    closest[(d3 >= 0) & (d4 <= d3)] = B
    closest[(d1 <= 0) & (d2 <= 0)] = A
    out[:] = np.linalg.norm(P - closest, axis=1)
    return out


def round_half_away(v):
    """roundf's rule (np.round rounds ties to even)."""
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def _clipped(lo_raw, hi_raw, N):
    """Box edges from the values before rounding; +-inf clip like any value beyond the grid."""
    with np.errstate(invalid="ignore"):
        lo = np.clip(round_half_away(np.clip(lo_raw, -4.0, N + 4.0)) - 1, 0, N - 1)
        hi = np.clip(round_half_away(np.clip(hi_raw, -4.0, N + 4.0)) + 1, -1, N - 1)
    # a lower edge beyond the grid leaves an empty box (lo > hi): keep it beyond rather than clipped onto the last voxel
    beyond = round_half_away(np.clip(lo_raw, -4.0, N + 4.0)) - 1 > N - 1
    lo = np.where(beyond, N, lo)
    return lo.astype(np.int64), hi.astype(np.int64)


def boxes(tri, resolution: int, extent: float):
    """(lo, hi, ambiguous): inclusive voxel index boxes [T, 3] (xyz; empty where lo > hi on an axis) of triangles [T, 3, 3], and the
    number of box edges within AMBIGUOUS voxels of a rounding tie that changes the clipped index."""
    N, cell, thr = grid(resolution, extent)
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        lo_raw = (tri.min(axis=1) - thr + extent) / cell
        hi_raw = (tri.max(axis=1) + thr + extent) / cell
    lo, hi = _clipped(lo_raw, hi_raw, N)
    lo_a, hi_a = _clipped(lo_raw - AMBIGUOUS, hi_raw - AMBIGUOUS, N)
    lo_b, hi_b = _clipped(lo_raw + AMBIGUOUS, hi_raw + AMBIGUOUS, N)
    return lo, hi, int((lo_a != lo_b).sum() + (hi_a != hi_b).sum())


def usable(positions, indices):
    """(triangles [T, 3, 3] float64 that the rule voxelizes, number skipped).  Degenerate is decided in fp32, the arithmetic of the
    API: the length of (v2 - v1) x (v3 - v1) or of an edge is not > 0 — zero, or NaN as it is for a NaN or infinite vertex and
    for differences that overflow."""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1)
    idx = idx[: idx.size // 3 * 3].reshape(-1, 3)
    in_range = (idx < len(pos)).all(axis=1)
    tri = pos[np.where(in_range[:, None], idx, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        edges = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], tri[:, 2] - tri[:, 1]], axis=1)
        length = lambda a: np.sqrt((a * a).sum(axis=-1, dtype=np.float32))
        keep = in_range & (length(np.cross(edges[:, 0], edges[:, 1])) > 0) & (length(edges) > 0).all(axis=1)  # NaN compares false
    return tri[keep].astype(np.float64), int((~keep).sum())


def well_conditioned(tri, cell: float):
    """bool [T]: finite, smallest angle >= MIN_ANGLE_DEG and shortest edge >= cell/4."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    ok = np.isfinite(tri).all(axis=(1, 2)) & (np.abs(tri) < 1e6).all(axis=(1, 2))
    t = np.where(ok[:, None, None], tri, 0.0)
    cosines, shortest = [], np.full(len(t), np.inf)
    for k in range(3):
        a, b = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
        la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
        shortest = np.minimum(shortest, la)
        with np.errstate(invalid="ignore", divide="ignore"):
            cosines.append(np.einsum("ij,ij->i", a, b) / (la * lb))
    with np.errstate(invalid="ignore"):
        return ok & (np.max(cosines, axis=0) <= np.cos(np.radians(MIN_ANGLE_DEG))) & (shortest >= cell / 4)


class Reference(NamedTuple):
    density: np.ndarray    # float64, [N, N, N] indexed [x, z, y], or [M] for `at`
    material: np.ndarray   # uint8, same shape
    covered: np.ndarray    # bool, same shape: inside at least one triangle's box
    ambiguous: int         # box edges next to a rounding tie: the comparison is only meaningful when 0
    lo: np.ndarray         # [T, 3] xyz
    hi: np.ndarray


def reference(tri, resolution: int, extent: float, at=None) -> Reference:
    """The rule of the module docstring over triangles [T, 3, 3] (already free of the skipped ones: usable()).  at: [M, 3] integer
    voxel indices (x, y, z) to evaluate instead of the whole grid."""
    N, cell, thr = grid(resolution, extent)
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    lo, hi, ambiguous = boxes(tri, resolution, extent)
    if at is None:
        shape = (N, N, N)
    else:
        at = np.asarray(at, np.int64).reshape(-1, 3)
        shape = (len(at),)
    density = np.full(shape, 2.0 * float(np.float32(extent)))
    covered = np.zeros(shape, bool)
    for t in range(len(tri)):
        if (lo[t] > hi[t]).any():
            continue
        if at is None:
            x, y, z = (np.arange(lo[t, a], hi[t, a] + 1) for a in range(3))
            X, Z, Y = np.meshgrid(x, z, y, indexing="ij")
            sel = (slice(x[0], x[-1] + 1), slice(z[0], z[-1] + 1), slice(y[0], y[-1] + 1))
            ijk = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
        else:
            sel = np.flatnonzero(((at >= lo[t]) & (at <= hi[t])).all(axis=1))
            if sel.size == 0:
                continue
            ijk = at[sel]
        d = np.empty(len(ijk))
        for a in range(0, len(ijk), 1 << 19):  # in pieces: the whole-grid triangle of a 513^3 sample is millions of points
            P = ijk[a:a + (1 << 19)] * cell - float(np.float32(extent))
            with np.errstate(invalid="ignore", over="ignore"):
                d[a:a + (1 << 19)] = point_triangle_distance(P, tri[t, 0], tri[t, 1], tri[t, 2]) / thr - 0.5
        d = np.where(np.isnan(d), np.inf, d)  # a triangle with an infinite vertex has no distance: it lowers nothing
        if at is None:
            density[sel] = np.minimum(density[sel], d.reshape(X.shape))
        else:
            density[sel] = np.minimum(density[sel], d)
        covered[sel] = True
    return Reference(density, (density <= 0).astype(np.uint8), covered, ambiguous, lo, hi)


def in_boxes(lo, hi, N: int, grow: int = 0) -> np.ndarray:
    """bool [N, N, N] indexed [x, z, y]: inside one of the boxes, each grown by `grow` voxels."""
    out = np.zeros((N, N, N), bool)
    for a, b in zip(lo, hi):
        if (a > b).any():
            continue
        a, b = np.maximum(a - grow, 0), np.minimum(b + grow, N - 1)
        out[a[0]:b[0] + 1, a[2]:b[2] + 1, a[1]:b[1] + 1] = True
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    name: str
    resolution: int
    extent: float
    positions: np.ndarray  # float32 [V, 3]
    indices: np.ndarray    # uint32 [I]
    skipped: int           # by the API's rule
    well: bool             # every usable triangle is well conditioned: the tolerance applies

    def triangles(self):
        return usable(self.positions, self.indices)[0]


def _case(name, resolution, extent, tri, well=True, positions=None, indices=None) -> Case:
    if positions is None:
        positions = np.ascontiguousarray(np.asarray(tri, np.float32).reshape(-1, 3))
        indices = np.arange(len(positions), dtype=np.uint32)
    kept, skipped = usable(positions, indices)
    if well:
        assert skipped == 0 and well_conditioned(kept, grid(resolution, extent)[1]).all(), name
        assert boxes(kept, resolution, extent)[2] == 0, name
    positions.setflags(write=False)
    indices.setflags(write=False)
    return Case(name, resolution, float(extent), positions, indices, skipped, well)


def kinds(tri, resolution, extent):
    """bool [T] each: (whole-grid box, crosses a face of the volume, clipped box one voxel thin, fully outside: empty box, box cut
    by the clip but not empty)."""
    N = grid(resolution, extent)[0]
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    lo, hi, _ = boxes(tri, resolution, extent)
    outside = (lo > hi).any(axis=1)
    whole = (lo == 0).all(axis=1) & (hi == N - 1).all(axis=1)
    mn, mx = tri.min(axis=1), tri.max(axis=1)
    crossing = ~outside & (((mn < -extent) & (mx > -extent)) | ((mn < extent) & (mx > extent))).any(axis=1)
    cell, thr = grid(resolution, extent)[1:]
    clipped = (round_half_away((mn - thr + extent) / cell) - 1 < 0) | (round_half_away((mx + thr + extent) / cell) + 1 > N - 1)
    thin = ~outside & ((lo == hi) & clipped).any(axis=1)
    return whole, crossing, thin, outside, ~outside & clipped.any(axis=1)


def required_kinds(resolution, span, extent=EXTENT):
    """Which of (crossing, thin, outside) the distribution of clipped_soup can give at all.  A vertex reaches at most
    (1.3 + span) * extent from the centre of the volume.  A box is empty when max + thr + extent < -1.5 cell, i.e. the whole triangle
    lies beyond (1 + (3 + 2 sqrt 3)/(N-1)) * extent, and one voxel thin at a face from (1 + (1 + 2 sqrt 3)/(N-1)) * extent on.  A kind
    is asked for when the room between that and the reach is at least a tenth of span * extent: with less, no draw in a million
    lands there.  So: crossing always; thin from resolution 2 (span 1.4) or 4 (span 0.15); outside from 3 or 4."""
    N = (1 << resolution) + 1
    room = lambda k: ((1.3 + span) - (1.0 + k / (N - 1))) / span >= 0.1
    return True, room(1 + 2 * np.sqrt(3.0)), room(3 + 2 * np.sqrt(3.0))


SOUPS = ((4, 1.4), (40, 1.4), (300, 0.15))


@functools.lru_cache(maxsize=None)
def clipped_soup(resolution: int, n: int, span: float, extent: float = EXTENT) -> Case:
    """n well-conditioned triangles: centres uniform in +-1.3 extent, vertices within +-span * extent of the centre, drawn from one
    seeded stream; a draw that is ill conditioned or has an ambiguous box edge is redrawn.  The first triangles kept are the
    stream's first face-crossing one, its first one-voxel-thin clipped one and its first fully outside one (required_kinds), the
    rest follow in stream order."""
    cell = grid(resolution, extent)[1]
    rng = np.random.RandomState(1000 * resolution + n)
    need = list(required_kinds(resolution, span, extent))
    special, rest = [], []
    for _ in range(64):
        c = rng.uniform(-1.3 * extent, 1.3 * extent, (8192, 1, 3))
        tri = (c + rng.uniform(-span * extent, span * extent, (8192, 3, 3))).astype(np.float32).astype(np.float64)
        ok = well_conditioned(tri, cell)
        ok &= _unambiguous(tri, resolution, extent)
        tri = tri[ok]
        k = kinds(tri, resolution, extent)
        taken = np.zeros(len(tri), bool)
        for j in range(3):
            free = np.flatnonzero(k[j + 1] & ~taken)
            if need[j] and free.size:
                special.append(tri[free[0]])
                taken[free[0]] = True
                need[j] = False
        rest.extend(tri[~taken][: max(0, n - len(rest))])
        if not any(need) and len(special) + len(rest) >= n:
            break
    assert not any(need), f"clipped_soup({resolution}, {n}, {span}): kinds missing {need}"
    tri = np.array(special + rest[: n - len(special)])
    assert len(tri) == n
    want = required_kinds(resolution, span, extent)
    have = kinds(tri, resolution, extent)
    assert all(have[j + 1].any() for j in range(3) if want[j])
    return _case(f"soup_{n}_{span}_res{resolution}", resolution, extent, tri)


def _unambiguous(tri, resolution, extent):
    """bool [T]: no box edge of the triangle is next to a rounding tie."""
    N, cell, thr = grid(resolution, extent)
    lo_raw = (tri.min(axis=1) - thr + extent) / cell
    hi_raw = (tri.max(axis=1) + thr + extent) / cell
    lo_a, hi_a = _clipped(lo_raw - AMBIGUOUS, hi_raw - AMBIGUOUS, N)
    lo_b, hi_b = _clipped(lo_raw + AMBIGUOUS, hi_raw + AMBIGUOUS, N)
    return (lo_a == lo_b).all(axis=1) & (hi_a == hi_b).all(axis=1)


def _redrawn(rng, draw, resolution, extent, n, well=True):
    """n triangles from draw(rng, count), each redrawn (same stream) until its box edges are unambiguous and, if asked, it is well
    conditioned."""
    cell = grid(resolution, extent)[1]
    out = []
    while len(out) < n:
        tri = draw(rng, 256).astype(np.float32).astype(np.float64)
        ok = _unambiguous(tri, resolution, extent)
        if well:
            ok &= well_conditioned(tri, cell)
        out.extend(tri[ok][: n - len(out)])
    return np.array(out)


@functools.lru_cache(maxsize=None)
def outside_only(resolution: int, near: bool, extent: float = EXTENT) -> Case:
    """near = False: triangles beyond thr + 2 cells of every face they face: every box is empty, the result is pure background.
    near = True: triangles parallel to the face x = +extent, between 0.3 thr and 0.8 thr outside it: they mark the layer x = N-1 (and
    whatever the +-1 voxel of the box adds) and nothing is solid but voxels of that layer."""
    N, cell, thr = grid(resolution, extent)
    rng = np.random.RandomState(77 + resolution + (100 if near else 0))
    if near:
        def draw(rng, count):
            t = rng.uniform(-0.8 * extent, 0.8 * extent, (count, 3, 3))
            t[:, :, 0] = extent + rng.uniform(0.3 * thr, 0.8 * thr, (count, 3))
            return t
        tri = _redrawn(rng, draw, resolution, extent, 6)
    else:
        gap = thr + 2.0 * cell
        def draw(rng, count):
            t = rng.uniform(-1.5 * extent, 1.5 * extent, (count, 3, 3))
            axis, side = rng.randint(0, 3, count), rng.choice([-1.0, 1.0], count)
            far = side[:, None] * (extent + gap + rng.uniform(0.01, 1.0, (count, 3)) * extent)
            t[np.arange(count), :, axis] = far
            return t
        tri = _redrawn(rng, draw, resolution, extent, 12)
        assert kinds(tri, resolution, extent)[3].all()
    return _case(f"outside_{'near' if near else 'far'}_res{resolution}", resolution, extent, tri)


@functools.lru_cache(maxsize=None)
def small_extent(resolution: int = 6, extent: float = 0.5) -> Case:
    """Extent 0.5: the background 2 * extent = 1 lies BELOW the densities of voxels far from a triangle inside its box (up to about
    2.2), so the background must win the minimum there."""
    def draw(rng, count):
        c = rng.uniform(-0.6 * extent, 0.6 * extent, (count, 1, 3))
        return c + rng.uniform(-0.3 * extent, 0.3 * extent, (count, 3, 3))
    tri = _redrawn(np.random.RandomState(5), draw, resolution, extent, 10)
    return _case(f"small_extent_res{resolution}", resolution, extent, tri)


@functools.lru_cache(maxsize=None)
def ill_conditioned(seed: int, resolution: int, extent: float = EXTENT) -> Case:
    """The kinds of tests/soak_voxelizer.py that no float64 reference can pin: seed % 3 == 0 sub-cell triangles, 1 needles (two
    vertices 1e-4 extent apart, every 7th exactly degenerate), 2 a torus with every 5th face twice.  Half of each kind is shifted so
    that it straddles a face of the volume.  Box edges are unambiguous (redrawn; torus faces next to a tie are left out)."""
    from volumetricraytracer_amd import voxelizer as vx

    N, cell, thr = grid(resolution, extent)
    rng = np.random.RandomState(seed)
    kind = seed % 3
    n = int(rng.choice([20, 100, 300]))

    def shifted(rng, t):
        """Every second triangle moved so that its first vertex lies within a cell of a face."""
        count = len(t)
        axis, side = rng.randint(0, 3, count), rng.choice([-1.0, 1.0], count)
        target = side * (extent + rng.uniform(-cell, cell, count))
        move = np.zeros((count, 1, 3))
        move[np.arange(count), 0, axis] = target - t[np.arange(count), 0, axis]
        move[::2] = 0.0
        return t + move

    if kind == 0:
        def draw(rng, count):
            c = rng.uniform(-0.9 * extent, 0.9 * extent, (count, 1, 3))
            return shifted(rng, c + rng.uniform(-0.4 * cell, 0.4 * cell, (count, 3, 3)))
        tri = _redrawn(rng, draw, resolution, extent, n, well=False)
    elif kind == 1:
        def draw(rng, count):
            a = rng.uniform(-0.9 * extent, 0.9 * extent, (count, 1, 3))
            b = rng.uniform(-0.9 * extent, 0.9 * extent, (count, 1, 3))
            return shifted(rng, np.concatenate([a, a + rng.uniform(-1e-4 * extent, 1e-4 * extent, (count, 1, 3)), b], axis=1))
        tri = _redrawn(rng, draw, resolution, extent, n, well=False)
        tri[::7, 1] = tri[::7, 0]
    else:
        pos, _, idx = vx.torus_mesh(0.4, 0.15, int(rng.randint(8, 24)), int(rng.randint(6, 14)))
        tri = pos[idx.reshape(-1, 3)].astype(np.float64) * (rng.uniform(1.3, 1.7) * extent)
        tri[1::2, :, int(rng.randint(0, 2))] += 0.9 * extent  # every second face is moved: that copy reaches through a face
        tri = tri.astype(np.float32).astype(np.float64)
        tri = tri[_unambiguous(tri, resolution, extent)]
        tri = np.concatenate([tri, tri[::5]], axis=0)
    case = _case(f"ill_{seed}_res{resolution}", resolution, extent, tri, well=False)
    assert boxes(case.triangles(), resolution, extent)[2] == 0
    k = kinds(case.triangles(), resolution, extent)
    assert (k[3] | k[4]).sum() >= len(k[0]) // 8, "ill_conditioned: too few triangles are cut by the clip"
    return case


@functools.lru_cache(maxsize=None)
def damaged_vertices(resolution: int = 5, extent: float = EXTENT) -> Case:
    """A good small mesh (an octahedron in the corner of negative coordinates) and, after it, triangles a damaged file can hold:
    vertices with NaN, +-inf, 3e38, 1e20 and -1e20, an index >= n_vertices, and two dangling indices at the end.  By the fp32 rule
    of usable() those whose cross product comes out NaN are skipped (NaN and infinite vertices, inf - inf), the others are voxelized
    with infinite distances.  The huge triangles keep y and z above 0.3 extent, so the good mesh's voxels are covered by
    well-conditioned triangles only."""
    e = extent
    c, r = np.array([-0.45 * e, -0.4 * e, -0.5 * e]), 0.33 * e
    good = [c + r * np.array(p, float) for p in ((1, 0, 0.03), (-1, 0.02, 0), (0, 1, 0.01), (0.04, -1, 0), (0, 0.05, 1), (0.02, 0, -1))]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    nan, inf = float("nan"), float("inf")
    bad = [[(nan, 0, 0), (10, 0, 0), (0, 10, 0)],                                  # skipped: NaN
           [(0, 0, 0), (10, nan, 0), (0, 10, nan)],                                # skipped: NaN
           [(inf, 0.5 * e, 0.5 * e), (10, 0.6 * e, 0.5 * e), (0, 0.5 * e, 0.7 * e)],       # one infinite vertex
           [(-inf, 0.5 * e, 0.5 * e), (inf, 0.6 * e, 0.5 * e), (0, 0.5 * e, inf)],         # three
           [(3e38, 3e38, 3e38), (3e38, 2e38, 3e38), (2e38, 3e38, 3e38)],           # far outside: differences overflow fp32
           [(3e38, 0.5 * e, 0.6 * e), (-3e38, 0.6 * e, 0.5 * e), (0, 0.5 * e, 3e38)],      # through the volume, edges overflow fp32
           [(1e20, 0.5 * e, 0.6 * e), (-1e20, 0.6 * e, 0.5 * e), (5, 0.55 * e, 1e20)],     # through the volume, squares overflow fp32
           [(-1e20, -1e20, -1e20), (-1e20, -1e20, -2e20), (-2e20, -1e20, -1e20)]]  # far outside
    positions = np.array(good + [p for t in bad for p in t], np.float32)
    idx = [i for f in faces for i in f]
    idx += list(range(6, 6 + 3 * len(bad)))
    idx += [0, 1, len(positions) + 3]  # out of range: skipped
    idx += [2, 3]                      # dangling: ignored
    case = _case(f"damaged_res{resolution}", resolution, extent, None, well=False, positions=positions, indices=np.array(idx, np.uint32))
    tri = case.triangles()
    cell = grid(resolution, extent)[1]
    ok = well_conditioned(tri, cell)
    assert ok[:8].all() and not ok[8:].any() and boxes(tri[:8], resolution, extent)[2] == 0
    return case


# ---- a case's expectations, computed once ---------------------------------------------------------------------------------------

class Expected(NamedTuple):
    ref: Reference          # over every usable triangle
    well_only: np.ndarray   # bool [N, N, N]: no ill-conditioned triangle's box, grown by a voxel, reaches the voxel
    check_material: np.ndarray  # bool [N, N, N]: |want| > tol


_EXPECTED = {}


def expected(case: Case) -> Expected:
    """Computed once per case (by name) and read-only."""
    if case.name not in _EXPECTED:
        _EXPECTED[case.name] = _expected(case)
    return _EXPECTED[case.name]


def _expected(case: Case) -> Expected:
    N, cell, thr = grid(case.resolution, case.extent)
    tri = case.triangles()
    ref = reference(tri, case.resolution, case.extent)
    ok = well_conditioned(tri, cell)
    well_only = ~in_boxes(ref.lo[~ok], ref.hi[~ok], N, grow=1)
    check = np.abs(ref.density) > tol(N, ref.density)
    if case.well:
        # chosen to stay within the share: decided by the reference alone
        assert (~check).sum() <= LEFT_OUT_SHARE * check.size, (case.name, int((~check).sum()))
    for a in (ref.density, ref.material, ref.covered, well_only, check):
        a.setflags(write=False)
    return Expected(ref, well_only, check)


@functools.lru_cache(maxsize=None)
def large_mesh(resolution: int, whole: bool = True, extent: float = EXTENT) -> Case:
    """<= 64 well-conditioned triangles for N = 257 and 513, drawn in cells of the grid from one stream whatever the
    resolution: 24 small ones in the far corner (box indices >= N - 25), 30 through the three far
    faces, and one large one — its box the whole grid, or (whole = False) the upper half of it, which leaves voxels outside every box."""
    N, cell, thr = grid(resolution, extent)
    rng = np.random.RandomState(8)

    def corner(rng, count):  # inside the far-corner box of 24^3 voxels, its own box included
        c = extent - rng.uniform(6.0, 14.0, (count, 1, 3)) * cell
        return c + rng.uniform(-3.0, 3.0, (count, 3, 3)) * cell

    def faces(rng, count):   # straddling one far face, anywhere on it
        c = rng.uniform(-0.9 * extent, 0.9 * extent, (count, 1, 3))
        c[np.arange(count), 0, rng.randint(0, 3, count)] = extent + rng.uniform(-2.0, 2.0, count) * cell
        return c + rng.uniform(-5.0, 5.0, (count, 3, 3)) * cell

    def large(rng, count):  # two opposite corners of the volume and a third one, each a little outside
        t = rng.uniform(1.0, 1.2, (count, 3, 3)) * extent * np.array([[-1, -1, -1], [1, 1, 1], [-1, 1, 0.3]], float)
        if not whole:
            t[:, 0, 2] = rng.uniform(-0.2 * extent, -0.1 * extent, count)
            t[:, 2, 2] = rng.uniform(0.0, 0.9 * extent, count)
        return t

    tri = np.concatenate([_redrawn(rng, corner, resolution, extent, 24), _redrawn(rng, faces, resolution, extent, 30),
                          _redrawn(rng, large, resolution, extent, 1)])
    lo, hi, amb = boxes(tri, resolution, extent)
    assert amb == 0 and len(tri) <= 64
    assert (lo[:24] >= N - 25).all() and (hi[:24] >= lo[:24]).all()
    assert (lo[-1, :2] == 0).all() and (hi[-1] == N - 1).all() and ((lo[-1, 2] == 0) if whole else (N // 3 < lo[-1, 2] < N // 2))
    return _case(f"large_res{resolution}", resolution, extent, tri)


@functools.lru_cache(maxsize=None)
def large_sample(resolution: int) -> np.ndarray:
    """[M, 3] xyz voxel indices, M >= 300 000: the far-corner 24^3 box, the two outermost layers of each face, a seeded sample."""
    N = (1 << resolution) + 1
    g = np.arange(N)
    c = np.arange(N - 24, N)
    parts = [np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)]
    A, B = (m.ravel() for m in np.meshgrid(g, g, indexing="ij"))
    for axis in range(3):
        for layer in (0, 1, N - 2, N - 1):
            p = np.empty((A.size, 3), np.int64)
            p[:, axis] = layer
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = A, B
            parts.append(p)
    parts.append(np.random.RandomState(resolution).randint(0, N, (100000, 3)))
    at = np.concatenate(parts)
    lin = np.unique((at[:, 0] * N + at[:, 1]) * N + at[:, 2])
    at = np.stack([lin // (N * N), (lin // N) % N, lin % N], axis=1)
    assert len(at) >= 300000
    at.setflags(write=False)
    return at
