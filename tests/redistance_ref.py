"""Plain-numpy reference of vrt_volume_redistance, written from the contract in include/vrt.h rather than from either C++ build: whole
[x, z, y] arrays, every operation an np.float32 operation in the header's parenthesisation (numpy's ufuncs round once per operation
and never fuse a multiply with an add; sqrt and division are correctly rounded), and the GLOBAL minimum over every surfel of the grid,
in chunks — no culling (cull=True applies the header's band + 1 rule instead, for the test that both give the same bits).

The state is what the device stores, as in brush_ref and fill_ref: `stored` is the DENSE buffer (F32: the densities; TEXEL16: the
integer field +-q as float32).  redistance() leaves it alone and returns an edited copy; material ids are not its business.

hand_made_fields() builds the 17^3 and 33^3 fields of tests/test_volume_redistance*.py: the smallest places the rule can go wrong."""
from __future__ import annotations

import numpy as np

from volume_ref import F32, TEXEL16, texel16_field

BOTH, OUTSIDE, INSIDE = 0, 1, 2
f32 = np.float32
AX = {0: 0, 1: 2, 2: 1}  # xyz axis -> axis of the [x, z, y] arrays
RADIUS = f32(0.75)


def decode(stored: np.ndarray, fmt: int) -> np.ndarray:
    """d, the density in the caller's units: the stored float, or stored * 0.01f (TEXEL16)."""
    return (stored * f32(0.01)).astype(f32) if fmt == TEXEL16 else stored


def clamped(d: np.ndarray) -> np.ndarray:
    """e = -0.0f when d is NaN, else fminf(fmaxf(d, -1e18f), 1e18f)."""
    with np.errstate(invalid="ignore"):
        e = np.fmin(np.fmax(d, f32(-1e18)), f32(1e18)).astype(f32)
    e[np.isnan(d)] = f32(-0.0)
    return e


def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def _neighbour(e: np.ndarray, axis: int, step: int):
    """(values, exists): the neighbour at index + step along the array axis; values are NaN where it lies beyond the grid."""
    out = np.full_like(e, np.nan)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
    else:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
    out[tuple(dst)] = e[tuple(src)]
    exists = np.zeros(e.shape, bool)
    exists[tuple(dst)] = True
    return out, exists


def surfels(e: np.ndarray, from_: int):
    """(mask [x, z, y], q int32 (K, 3) xyz, c float32 (K, 3) xyz, n float32 (K, 3) xyz) of the surfels of the whole grid, in array
    order of their samples."""
    out = e > f32(0.0)
    sigma = np.where(out, f32(1.0), f32(-1.0)).astype(f32)
    phi = (sigma * e).astype(f32)
    interface = np.zeros(e.shape, bool)
    s, direction = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            ep, hp = _neighbour(e, AX[a], +1)
            em, hm = _neighbour(e, AX[a], -1)
            interface |= (hp & ((ep > f32(0.0)) != out)) | (hm & ((em > f32(0.0)) != out))
            wp = (phi - sigma * ep).astype(f32)  # NaN where the neighbour does not exist: fmax passes over it
            wm = (phi - sigma * em).astype(f32)
            s.append(np.fmax(np.fmax(wp, wm), f32(0.0)).astype(f32))
            direction.append(np.where(hm & (~hp | (wm > wp)), f32(-1.0), f32(1.0)).astype(f32))
        mask = interface & {BOTH: np.ones(e.shape, bool), OUTSIDE: out, INSIDE: ~out}[from_]
        x, z, y = np.nonzero(mask)
        q = np.stack([x, y, z], axis=1).astype(np.int32)
        sk = [sa[mask] for sa in s]
        dk = [da[mask] for da in direction]
        ph = phi[mask]
        G = _dot(sk[0], sk[1], sk[2], sk[0], sk[1], sk[2]).astype(f32)
        root = np.sqrt(G).astype(f32)
        c = np.stack([(q[:, a].astype(f32) + dk[a] * ((ph * sk[a]) / G)).astype(f32) for a in range(3)], axis=1)
        n = np.stack([(dk[a] * (sk[a] / root)).astype(f32) for a in range(3)], axis=1)
    return mask, q, c, n


def min_d2(p: np.ndarray, q: np.ndarray, c: np.ndarray, n: np.ndarray, reach=None, budget: int = 1 << 22) -> np.ndarray:
    """The smallest D2 of every sample p (M, 3 int xyz) over the surfels (inf without any); reach: skip the surfels whose sample lies
    more than that many indices from p on some axis."""
    best = np.full(p.shape[0], np.inf, f32)
    K = q.shape[0]
    if K == 0:
        return best
    rows = max(1, budget // K)
    cx, cy, cz, nx, ny, nz = (v[None, :] for v in (c[:, 0], c[:, 1], c[:, 2], n[:, 0], n[:, 1], n[:, 2]))
    with np.errstate(all="ignore"):
        for at in range(0, p.shape[0], rows):
            pp = p[at:at + rows]
            pf = pp.astype(f32)
            vx, vy, vz = pf[:, 0:1] - cx, pf[:, 1:2] - cy, pf[:, 2:3] - cz
            h = _dot(vx, vy, vz, nx, ny, nz)
            vv = _dot(vx, vy, vz, vx, vy, vz)
            hh = h * h
            r = np.sqrt(np.fmax(vv - hh, f32(0.0)))
            u = np.fmax(r - RADIUS, f32(0.0))
            d2 = (hh + u * u).astype(f32)
            if reach is not None:
                for a in range(3):
                    d2[np.abs(pp[:, a:a + 1] - q[None, :, a]) > reach] = np.inf
            best[at:at + rows] = np.fmin.reduce(d2, axis=1, initial=np.inf)
    return best


def redistance(stored: np.ndarray, fmt: int, band: int, from_: int, unit, lo=None, hi=None, cull: bool = False):
    """(stored', info): a copy with the samples lo..hi (xyz, inclusive; the whole grid without a box) holding the banded signed
    distance m — its texel in TEXEL16; info = {"written", "near", "surfels", "lo", "hi"} as vrt_redistance_result reports."""
    assert fmt in (F32, TEXEL16) and stored.dtype == np.float32 and 1 <= band <= 15
    N = stored.shape[0]
    lo = (0, 0, 0) if lo is None else tuple(int(v) for v in lo)
    hi = (N - 1,) * 3 if hi is None else tuple(int(v) for v in hi)
    e = clamped(decode(stored, fmt))
    mask, q, c, n = surfels(e, from_)
    grown = np.ones(len(q), bool)
    for a in range(3):
        grown &= (q[:, a] >= lo[a] - (band + 1)) & (q[:, a] <= hi[a] + (band + 1))
    box = (slice(lo[0], hi[0] + 1), slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1))
    x, z, y = np.meshgrid(*(np.arange(lo[a], hi[a] + 1) for a in (0, 2, 1)), indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int32)
    best = min_d2(p, q, c, n, reach=band + 1 if cull else None).reshape(x.shape)
    with np.errstate(all="ignore"):
        D = np.fmin(np.sqrt(best), f32(band)).astype(f32)
        Du = (D * f32(unit)).astype(f32)
    m = np.where(e[box] > f32(0.0), Du, -Du).astype(f32)
    out = stored.copy()
    out[box] = texel16_field(m) if fmt == TEXEL16 else m
    info = {"written": int(D.size), "near": int((D < f32(band)).sum()), "surfels": int(grown.sum()), "lo": lo, "hi": hi}
    return out, info


# ---- hand-made fields ------------------------------------------------------------------------------------------------------------

def _index(N):
    i = np.arange(N, dtype=np.float64)
    return i[:, None, None], i[None, None, :], i[None, :, None]  # x, y, z broadcast over [x, z, y]


def sphere_field(N: int, centre, radius: float, unit: float) -> np.ndarray:
    """A true signed distance (density units) to a sphere given in cells."""
    x, y, z = _index(N)
    return ((np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius) * unit).astype(f32)


OBLIQUE_NORMAL = (0.48, 0.6, 0.64)  # a unit vector oblique to all axes: 0.2304 + 0.36 + 0.4096 = 1
OBLIQUE_POINT = (16.2, 15.7, 16.4)


def oblique_distance(N: int) -> np.ndarray:
    """The signed distance (cells, float64) to the plane through OBLIQUE_POINT."""
    x, y, z = _index(N)
    a, o = OBLIQUE_NORMAL, OBLIQUE_POINT
    return a[0] * (x - o[0]) + a[1] * (y - o[1]) + a[2] * (z - o[2]) + np.zeros((N, N, N))


def hand_made_fields() -> dict:
    """name -> density [x, z, y] (density units of a volume of extent 100 with density_scale 1)."""
    N = 17
    x, y, z = _index(N)
    full = lambda v: (v + np.zeros((N, N, N))).astype(f32)
    fields = {"no surfel": full(2.5), "all inside": full(-2.5)}
    # a slab one sample thick across x with equal values on both sides (w+ == w-: the tie goes to +1), and one across y with unequal ones
    slab = full(1.0)
    slab[8, :, :] = f32(-0.25)
    slab[:, :, 3] = f32(-0.5)
    slab[:, :, 2] = f32(0.75)
    fields["slab"] = slab
    # zero samples on the face x = 0 (inside, without a neighbour at -1) and an inside layer on the face y = N - 1
    face = full(0.5 * x)
    face[:, :, N - 1] = f32(-0.3)
    fields["face"] = face
    # a plane z = 8.3 with odd values next to it
    odd = full((z - 8.3) * 0.7)
    for k, value in enumerate((np.nan, 0.0, -0.0, np.inf, -np.inf, 1e30, -1e30)):
        odd[2 * k + 1, 8, 3] = f32(value)   # z = 8: below the plane
        odd[2 * k + 1, 9, 11] = f32(value)  # z = 9: above it
    fields["odd values"] = odd
    fields["small sphere"] = sphere_field(N, (8.3, 7.8, 8.1), 4.3, 1.0)
    fields["oblique plane"] = (oblique_distance(33) * 1.7).astype(f32)  # linear, in some unit of its own
    return fields
