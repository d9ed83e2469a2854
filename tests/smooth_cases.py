"""The cases that tests/test_volume_smooth.py (host pass) and tests/test_volume_smooth_gpu.py (device) share: the fields, the records
of the sweep and the reference's results (tests/smooth_ref.py), each computed once and never written to afterwards."""
from __future__ import annotations

import functools

import numpy as np

import smooth_ref as S
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

FORMATS = (R.F32, R.TEXEL16)
SIZES = (9, 17, 33)
SHAPES = (_abi.BRUSH_SPHERE, _abi.BRUSH_BOX, _abi.BRUSH_CAPSULE)
ITERATIONS = (1, 2, 3, 16)  # odd and even counts end in different copies
STRENGTHS = ((0.0, 1.0), (1.0, 0.25), (1.0, 0.5))  # (rebound, strength): strength 1 without a rebound, 0.25 and 0.5 with
MATERIALS = (-1, 7)


def resolution(N: int) -> int:
    return int(N - 1).bit_length() - 1


def volume(N: int, table: bool = False) -> v.VVoxelVolume:
    """An empty volume of N^3 samples whose cell is 1 and whose density unit is a cell, with (step_max > 0) or without the
    empty-space tables on the device."""
    vol = v.VVoxelVolume(resolution(N), (N - 1) / 2.0)
    assert vol.N == N
    vol.step_max = 1.5 * vol.GetCellSize() if table else 0.0
    return vol


def sphere_radius(N: int) -> float:
    return 0.325 * (N - 1)


@functools.lru_cache(maxsize=None)
def field(N: int, fmt: int):
    """(stored, material): a sphere of 0.325 (N - 1) cells with +-0.3 cells of noise, as a slot of the format stores it, and ids that
    differ from sample to sample."""
    d = S.noisy_sphere(N, sphere_radius(N), 0.3, seed=N)
    stored = R.dense_field(d, fmt)
    material = ((np.arange(N ** 3, dtype=np.int64).reshape(N, N, N) * 7) % 5).astype(np.uint8)
    for a in (stored, material):
        a.setflags(write=False)
    return stored, material


def shape_record(N: int, shape: int, **kw):
    """The sweep's region of a shape, across the sphere's surface: a ball of 0.8 R centred on the surface (off the sample lattice), a
    rounded box over the surface's +y cap, a capsule from the -x side of the surface to its +y side."""
    c, r = (N - 1) / 2.0, sphere_radius(N)
    if shape == _abi.BRUSH_SPHERE:
        return v.smooth_record(shape, (c + r, c + 0.3, c - 0.2), (0.0, 0.0, 0.0), 0.8 * r, **kw)
    if shape == _abi.BRUSH_BOX:
        return v.smooth_record(shape, (c + 0.2, c + r, c - 0.3), (0.7 * r, 0.6 * r, 0.5 * r), 0.2 * r, **kw)
    return v.smooth_record(shape, (c - r, c + 0.1, c + 0.5 * r), (c + 0.2 * r, c + r, c - 0.2), 0.45 * r, **kw)


def sweep(N: int):
    """[(what, record)]: shapes x iteration counts x (rebound, strength), the material and the falloff cycling."""
    out = []
    for shape in SHAPES:
        for it in ITERATIONS:
            for rebound, strength in STRENGTHS:
                n = len(out)
                material, falloff = MATERIALS[n % 2], (2.0, 0.75, 50.0)[n % 3]
                rec = shape_record(N, shape, strength=strength, iterations=it, falloff=falloff, rebound=rebound, material=material)
                out.append((f"shape {shape}, {it} iterations, rebound {rebound}, strength {strength}, material {material}, falloff {falloff}", rec))
    return out


def key_of(rec):
    return (rec.shape, rec.iterations, tuple(rec.a), tuple(rec.b), rec.radius, rec.strength, rec.falloff, rec.rebound, rec.material)


_results = {}


def reference(stored, material, fmt: int, rec, tag):
    """smooth_ref.smooth, kept per (tag, record): (stored', material', result), read-only."""
    key = (tag, fmt, key_of(rec))
    if key not in _results:
        d, m, info = S.smooth(stored, material, fmt, rec)
        for a in (d, m):
            a.setflags(write=False)
        _results[key] = (d, m, info)
    return _results[key]


def sweep_reference(N: int, fmt: int, rec):
    stored, material = field(N, fmt)
    return reference(stored, material, fmt, rec, ("sweep", N))


# ---- resolutions 0, 1, 2 -------------------------------------------------------------------------------------------------------------

SMALL = (2, 3, 5)  # one brick, one tile of a pass, a work box that is the whole grid


def small_cases(N: int):
    """[(what, record)] for the grids of 2, 3 and 5 samples: a box over the whole grid (every neighbour of a face sample beyond it is
    the sample itself), a ball about a corner and a capsule along an edge."""
    c = (N - 1) / 2.0
    return [("whole-grid box, 3 iterations", v.smooth_record(_abi.BRUSH_BOX, (c, c, c), (N, N, N), 0.0, strength=1.0, iterations=3, falloff=0.5, material=6)),
            ("whole-grid box, rebound", v.smooth_record(_abi.BRUSH_BOX, (c, c, c), (N, N, N), 0.5, strength=0.5, iterations=2, falloff=2.0, rebound=1.0)),
            ("corner ball", v.smooth_record(_abi.BRUSH_SPHERE, (N - 1.2, 0.1, N - 0.9), (0, 0, 0), 1.6, strength=0.5, iterations=16, falloff=1.0, material=0)),
            ("edge capsule", v.smooth_record(_abi.BRUSH_CAPSULE, (0.0, 0.2, 0.1), (N - 1.0, 0.0, 0.3), 0.9, strength=0.25, iterations=1, falloff=0.3,
                                             rebound=0.5, material=255))]
