"""Plain-numpy reference of vrt_volume_smooth, written from the contract in include/vrt.h rather than from the kernels: whole
[x, z, y] arrays, the whole volume, no box.  Every operation is an np.float32 operation in the header's parenthesisation (numpy's
ufuncs round once per operation and never fuse a multiply with an add; sqrt and division are correctly rounded); the neighbour beyond
the grid is the sample itself through np.pad(mode="edge").

The state is what the device stores: `stored` is the DENSE buffer (F32: the densities; TEXEL16: the integer field +-q as float32)
and `material` the material ids.  smooth() leaves both alone and returns the edited copies with what vrt_brush_result reports.

Also what the rule is measured with (tools/smooth_probe.py, and one test of the reference itself): a noisy sphere and the radial error
of its zero crossings on grid edges."""
from __future__ import annotations

import numpy as np

from brush_ref import brush_distance, decode
from volume_ref import F32, TEXEL16, texel16_field

f32 = np.float32
SIXTH = np.array([0x3E2AAAAB], np.uint32).view(np.float32)[0]  # 0.16666667f


def weights(rec, N: int):
    """Step 1: (region mask, w) over the grid; w is only meaningful inside the region."""
    s = brush_distance(rec, N)
    with np.errstate(all="ignore"):
        region = s < f32(0.0)
        w = f32(rec.strength) * np.fmin((-s) / f32(rec.falloff), f32(1.0))
    return region, w.astype(f32)


def one_pass(f: np.ndarray, region: np.ndarray, u: np.ndarray) -> np.ndarray:
    """Step 3: every read sees f; samples outside the region keep their value."""
    p = np.pad(f, 1, mode="edge")
    c = slice(1, -1)
    with np.errstate(all="ignore"):
        L = ((p[:-2, c, c] + p[2:, c, c]) + (p[c, c, :-2] + p[c, c, 2:])) + (p[c, :-2, c] + p[c, 2:, c])  # x, then y, then z
        avg = L * SIXTH
        moved = f + (u * (avg - f))
    assert moved.dtype == np.float32
    return np.where(region, moved, f)


def relax(f0: np.ndarray, rec) -> tuple:
    """Steps 1, 3 and 4 on a decoded field: (region, the field after the last pass)."""
    region, w = weights(rec, f0.shape[0])
    f = f0
    for _ in range(int(rec.iterations)):
        f = one_pass(f, region, w)
        if rec.rebound > 0:
            with np.errstate(all="ignore"):
                f = one_pass(f, region, -(f32(rec.rebound) * w))
    return region, f


def smooth(stored: np.ndarray, material: np.ndarray, fmt: int, rec) -> tuple:
    """(stored', material', {"written", "lo", "hi"}) — lo > hi when nothing was written."""
    assert fmt in (F32, TEXEL16) and stored.dtype == np.float32 and material.dtype == np.uint8
    N = stored.shape[0]
    region, m = relax(decode(stored, fmt), rec)
    value = texel16_field(m) if fmt == TEXEL16 else m
    written = region & (m == m) & (value.view(np.uint32) != stored.view(np.uint32))  # step 5: never NaN, only bits that differ
    out_d, out_m = stored.copy(), material.copy()
    out_d[written] = value[written]
    if rec.material >= 0:  # step 6
        out_m[written] = np.where(m <= f32(0.0), np.uint8(rec.material), np.uint8(0))[written]
    if not written.any():
        return out_d, out_m, {"written": 0, "lo": (N, N, N), "hi": (-1, -1, -1)}
    x, z, y = np.nonzero(written)
    return out_d, out_m, {"written": int(written.sum()), "lo": (int(x.min()), int(y.min()), int(z.min())),
                          "hi": (int(x.max()), int(y.max()), int(z.max()))}


# ---- what the rule is worth ---------------------------------------------------------------------------------------------------------

def noisy_sphere(N: int, radius: float, noise: float, seed: int = 7, centre=None) -> np.ndarray:
    """The signed distance (cells) to a sphere about the grid's centre plus uniform noise of +-noise per sample, float32 [x, z, y]."""
    c = ((N - 1) / 2.0,) * 3 if centre is None else centre
    i = np.arange(N, dtype=np.float64)
    x, z, y = i[:, None, None], i[None, :, None], i[None, None, :]
    d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius
    rng = np.random.default_rng(seed)
    return (d + rng.uniform(-noise, noise, d.shape)).astype(np.float32)


def crossing_errors(f: np.ndarray, radius: float, centre=None) -> tuple:
    """(RMS, mean) of the radial error, in cells, of the zero crossings on grid edges: on every edge whose two samples differ in sign
    the crossing is interpolated linearly, and its error is its distance from the centre minus the radius."""
    N = f.shape[0]
    c = np.array(((N - 1) / 2.0,) * 3 if centre is None else centre)  # xyz
    f = f.astype(np.float64)
    grid = np.stack(np.meshgrid(*[np.arange(N, dtype=np.float64)] * 3, indexing="ij"), -1)  # [x, z, y] -> (x, z, y)
    centre_xzy = np.array([c[0], c[2], c[1]])
    errs = []
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        fa, fb = f[tuple(a)], f[tuple(b)]
        cross = (fa <= 0) != (fb <= 0)
        t = fa[cross] / (fa[cross] - fb[cross])
        p = grid[tuple(a)][cross] + t[:, None] * (grid[tuple(b)][cross] - grid[tuple(a)][cross])
        errs.append(np.linalg.norm(p - centre_xzy, axis=1) - radius)
    e = np.concatenate(errs)
    return float(np.sqrt(np.mean(e ** 2))), float(np.mean(e))
