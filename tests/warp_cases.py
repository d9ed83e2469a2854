"""The cases that tests/test_volume_warp.py (host pass) and tests/test_volume_warp_gpu.py (device) share: the records of the sweep,
the named cases and the reference's results (tests/warp_ref.py), each computed once and never written to afterwards.  The fields, the
volumes and the regions are those of tests/smooth_cases.py."""
from __future__ import annotations

import functools
import math

import numpy as np

import smooth_cases as SK
import smooth_ref as S
import volume_ref as R
import volumetricraytracer_amd as v
import warp_ref as W
from volumetricraytracer_amd import _abi

FORMATS = SK.FORMATS
SIZES = SK.SIZES
SHAPES = SK.SHAPES
MATERIALS = (-1, 7, -2)
FALLOFFS = (0.75, 2.0, 50.0)
field, volume = SK.field, SK.volume


def region_of(N: int, shape: int) -> dict:
    """The sweep's region of a shape, as smooth_cases.shape_record places it: the keywords of warp_record."""
    r = SK.shape_record(N, shape)
    return dict(shape=shape, a=tuple(r.a), b=tuple(r.b), radius=r.radius)


def region_centre(region: dict):
    a, b = np.array(region["a"], np.float64), np.array(region["b"], np.float64)
    return tuple((a + b) / 2.0) if region["shape"] == _abi.BRUSH_CAPSULE else tuple(a)


def grab(vec):
    return v.warp_from_motion((0.0, 0.0, 0.0), translation=vec)[0]


def motions(region: dict):
    """[(name, keywords of warp_record)]: the sweep's motions about a region."""
    c = region_centre(region)
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    twist = tuple(axis * math.sin(0.2)) + (math.cos(0.2),)  # 0.4 rad
    flat = np.array(W.IDENTITY, np.float64).reshape(3, 4)
    flat[2] = (0.0, 0.0, 0.0, c[2] + 0.3)  # every source on the plane z = const: a singular matrix
    scaled = v.warp_from_motion(c, scale=1.25)
    return [("grab by (2, -1, 1)", dict(pull=grab((2.0, -1.0, 1.0)))),
            ("grab by (1.3, -0.6, 0.4)", dict(pull=grab((1.3, -0.6, 0.4)))),
            ("twist of 0.4 rad", dict(pull=v.warp_from_motion((c[0] + 0.3, c[1] - 0.2, c[2] + 0.4), rotation=twist)[0], strength=0.7)),
            ("scale by 1.25", dict(pull=scaled[0], length_scale=scaled[1])),
            ("inflate by 1.5", dict(inflate=1.5)),
            ("inflate by -0.7", dict(inflate=-0.7)),
            ("flatten onto a plane", dict(pull=flat))]


def sweep(N: int):
    """[(what, record)]: shapes x motions, the material and the falloff cycling."""
    out = []
    for shape in SHAPES:
        region = region_of(N, shape)
        for name, fields in motions(region):
            n = len(out)
            material, falloff = MATERIALS[n % 3], FALLOFFS[(n // 3 + n) % 3]
            out.append((f"shape {shape}, {name}, material {material}, falloff {falloff}", v.warp_record(falloff=falloff, material=material, **region, **fields)))
    return out


def key_of(rec):
    return (rec.shape, rec.material, tuple(rec.a), tuple(rec.b), rec.radius, rec.strength, rec.falloff, tuple(rec.pull), rec.length_scale, rec.inflate)


_results = {}


def reference(stored, material, fmt: int, rec, tag):
    """warp_ref.warp, kept per (tag, record): (stored', material', result, density writes), read-only."""
    key = (tag, fmt, key_of(rec))
    if key not in _results:
        d, m, info, density = W.warp(stored, material, fmt, rec)
        for a in (d, m):
            a.setflags(write=False)
        _results[key] = (d, m, info, density)
    return _results[key]


def sweep_reference(N: int, fmt: int, rec):
    stored, material = field(N, fmt)
    return reference(stored, material, fmt, rec, ("sweep", N))


def read_only(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the named cases: (stored, material, record) ------------------------------------------------------------------------------------

def identity_cases(N: int = 17):
    """An identity record over a whole-grid box, for both material modes that read ids: nothing may be written, in either format."""
    c = (N - 1) / 2.0
    return [v.warp_record(_abi.BRUSH_BOX, (c, c, c), (N, N, N), 0.0, falloff=1.0, material=m) for m in (_abi.WARP_MATERIAL_KEEP, _abi.WARP_MATERIAL_SOURCE)]


COPY_GRAB = (3, 0, -2)


def copy_case():
    """33^3 F32, a sphere SDF of 8 cells, a ball region of 14 cells about the centre, falloff 2, strength 1, a grab by (3, 0, -2)."""
    N, c = W.WORTH_N, (W.WORTH_N - 1) / 2.0
    stored = S.noisy_sphere(N, W.WORTH_RADIUS, 0.0)
    material = (stored <= 0).astype(np.uint8)
    rec = v.warp_record(_abi.BRUSH_SPHERE, (c, c, c), (0, 0, 0), W.WORTH_REGION, pull=grab(COPY_GRAB), falloff=W.WORTH_FALLOFF, material=_abi.WARP_MATERIAL_SOURCE)
    return read_only(stored, material) + (rec,)


def jacobi_case(fmt: int):
    """65^3, a ball of 20 cells about (34.5, 29.4, 34.9) grabbed by (9.3, -4.2, 6.6) at falloff 14: one-to-one by the slope rule
    (1.5 / 14 * 12.2 = 0.8 < 1).  The box starts on samples that are multiples of neither 4 nor 8, spans several workgroups and bricks
    per axis, and sources lie in other bricks than their destinations."""
    N = 65
    stored = R.dense_field(S.noisy_sphere(N, SK.sphere_radius(N), 0.3, seed=N), fmt)
    material = ((np.arange(N ** 3, dtype=np.int64).reshape(N, N, N) * 7) % 5).astype(np.uint8)
    rec = v.warp_record(_abi.BRUSH_SPHERE, (34.5, 29.4, 34.9), (0, 0, 0), 20.0, pull=grab((9.3, -4.2, 6.6)), falloff=14.0, material=_abi.WARP_MATERIAL_SOURCE)
    return read_only(stored, material) + (rec,)


def clamp_case(fmt: int):
    """33^3, a ball of 6 cells about (16.2, 15.7, 2.5) grabbed by (0, 0, +5): sources below z = 0 are the face z = 0."""
    N = 33
    rng = np.random.default_rng(11)
    stored = R.dense_field(rng.uniform(-3.0, 3.0, (N, N, N)).astype(np.float32), fmt)
    material = (stored <= 0).astype(np.uint8)
    rec = v.warp_record(_abi.BRUSH_SPHERE, (16.2, 15.7, 2.5), (0, 0, 0), 6.0, pull=grab((0.0, 0.0, 5.0)), falloff=2.0, material=3)
    return read_only(stored, material) + (rec,)


def material_only_case(N: int = 17):
    """F32, the constant density -1, ids that differ from sample to sample, a grab by (2, 1, 0) that takes the source's ids: no density
    can change."""
    stored = np.full((N, N, N), -1.0, np.float32)
    material = np.array(field(N, R.F32)[1])
    c = (N - 1) / 2.0
    rec = v.warp_record(_abi.BRUSH_SPHERE, (c + 0.3, c, c - 0.2), (0, 0, 0), 5.0, pull=grab((2.0, 1.0, 0.0)), falloff=2.0, material=_abi.WARP_MATERIAL_SOURCE)
    return read_only(stored, material) + (rec,)


SMALL = SK.SMALL


@functools.lru_cache(maxsize=None)
def small_field(N: int, fmt: int):
    """(stored, material): extreme_cases.small_field — seeded densities of both signs with a NaN, a +0 and a -0 sample — with the NaN
    moved from the sample (1, 1, 1), a corner of every cell of a 3^3 grid (there every trilinear value would be a NaN and nothing could
    ever be written), to the far corner (N - 1, 0, N - 1) of the array, which only one cell touches."""
    import extreme_cases as X
    import fill_ref as F
    d = np.array(X.random_field(N))
    if N >= 3:
        assert np.isnan(d[1, 1, 1])
        d[1, 1, 1], d[N - 1, 0, N - 1] = d[N - 1, 0, N - 1], d[1, 1, 1]
    return read_only(R.dense_field(d, fmt), F.hand_made_material(d))


def small_cases(N: int):
    """[(what, record)] for the grids of 2, 3 and 5 samples: a grab and an inflate in each of smooth_cases.small_cases' regions."""
    out = []
    for n, (what, r) in enumerate(SK.small_cases(N)):
        region = dict(shape=r.shape, a=tuple(r.a), b=tuple(r.b), radius=r.radius)
        out.append((f"{what}, grab", v.warp_record(pull=grab((0.6, -0.3, 1.0)), falloff=0.5, material=MATERIALS[n % 3], **region)))
        out.append((f"{what}, inflate", v.warp_record(inflate=0.4, falloff=1.0, material=MATERIALS[(n + 1) % 3], **region)))
    return out
