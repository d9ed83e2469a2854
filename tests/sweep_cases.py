"""The seeded scenes and records that the sweep tests share: test_query_sweeps.py (no GPU: the reference's own worth, and that the
float64 reference leaves few enough records undecided on the inputs of the GPU test) and test_query_sweeps_gpu.py."""
from __future__ import annotations

import numpy as np

import points_ref as P
import volumetricraytracer_amd as v
from volume_ref import dense_field
from volumetricraytracer_amd import _abi

f32 = np.float32
FORMATS = [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16]
EXTENT = 3.3
RADII_CELLS = (0.0, 0.5, 1.5)


def ref_scene(sc):
    """(slots, instances) of points_ref from the scene as the renderer uploads it."""
    slots = [P.Slot(dense_field(vol.density, vol.device_format), np.asarray(vol.material_id, np.uint8), vol.device_format, vol.VolumeExtends,
                    vol.density_scale, vol.step_max) for vol in sc.volumes()]
    a = sc.to_abi()
    inst = [P.Instance(a.instances[i].volume_slot, tuple(a.instances[i].position), tuple(a.instances[i].rotation), tuple(a.instances[i].scale))
            for i in range(a.n_instances)]
    return slots, inst


def volume(res, extent, fn=None, fmt=_abi.FORMAT_F32, density=None):
    vol = v.VVoxelVolume(res, extent)
    if fn is not None:
        vol.fill(fn)
    if density is not None:
        vol.density = np.ascontiguousarray(density, f32)
        with np.errstate(invalid="ignore"):
            vol.material_id = (vol.density <= 0).astype(np.uint8) * 3
    return vol.set_device_format(fmt)


def sphere_fn(radius, centre=(0.0, 0.0, 0.0)):
    cx, cy, cz = (f32(c) for c in centre)
    return lambda X, Y, Z: np.sqrt(((X - cx) * (X - cx) + (Y - cy) * (Y - cy)) + (Z - cz) * (Z - cz)).astype(f32) - f32(radius)


def random_field(N, seed):
    """Values of a few tenths of the extent with NaNs and -0 among them: no distance, but every bit of it is pinned."""
    rng = np.random.default_rng(seed)
    d = (rng.normal(size=(N, N, N)) * 0.8 + 0.5).astype(f32)
    flat = d.reshape(-1)
    flat[rng.choice(flat.size, max(3, flat.size // 60), replace=False)] = np.nan
    flat[rng.choice(flat.size, max(3, flat.size // 60), replace=False)] = f32(-0.0)
    return d


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# -- 1. one pinned instance ------------------------------------------------------------------------------------------------------------
def pinned_scene(res, fmt, field):
    N = (1 << res) + 1
    if field == "sphere":
        vol = volume(res, EXTENT, sphere_fn(0.6 * EXTENT), fmt)
    else:
        vol = volume(res, EXTENT, None, fmt, random_field(N, 100 + res))
        vol.material_id = np.random.default_rng(res).integers(0, 256, (N, N, N)).astype(np.uint8)
    return v.VScene(Objects=[v.VVoxelObject(Volume=vol)]), vol


BAD = 9  # the records that pinned_records puts last: none of them is an error, each is a miss with steps 0


def pinned_records(vol, seed):
    """Starts outside, in the box and in the solid; directions at random, parallel to the faces, and along the faces themselves; radii
    0, half a cell and 1.5 cells in turn; t_max long, short and 0; and the BAD records."""
    E, cell = f32(vol.VolumeExtends), float(vol.GetCellSize())
    rng = np.random.default_rng(seed)
    o = [rng.uniform(-1.8 * EXTENT, 1.8 * EXTENT, (900, 3)), rng.uniform(-EXTENT, EXTENT, (300, 3)), unit(rng, 150) * rng.uniform(0, 0.55 * EXTENT, (150, 1))]
    d = [unit(rng, 900) * rng.uniform(0.1, 10.0, (900, 1)), unit(rng, 300), unit(rng, 150)]
    # towards the volume from far outside, so that hits from outside are many
    far = unit(rng, 400) * rng.uniform(1.9 * EXTENT, 3.0 * EXTENT, (400, 1))
    o.append(far)
    d.append(-far + rng.normal(size=(400, 3)) * 0.9)
    # parallel to an axis
    axis = np.eye(3)[rng.integers(0, 3, 200)] * rng.choice([-1.0, 1.0], (200, 1))
    o.append(rng.uniform(-1.5 * EXTENT, 1.5 * EXTENT, (200, 3)))
    d.append(axis)
    # on a face, moving in it
    on = rng.uniform(-EXTENT, EXTENT, (120, 3))
    along = unit(rng, 120)
    a = rng.integers(0, 3, 120)
    on[np.arange(120), a] = rng.choice([-1.0, 1.0], 120) * float(E)
    along[np.arange(120), a] = 0.0
    o.append(on)
    d.append(along)
    o, d = np.concatenate(o).astype(f32), np.concatenate(d).astype(f32)
    n = len(o)
    radius = (np.array(RADII_CELLS)[np.arange(n) % 3] * cell).astype(f32)
    t_max = np.full(n, 10000.0, f32)
    t_max[::5] = rng.uniform(0.0, 2.0 * EXTENT, len(t_max[::5])).astype(f32)
    t_max[7::50] = 0.0
    rec = v.make_sweeps(o, d, radius, t_max)
    nan, inf = f32(np.nan), f32(np.inf)
    bad = v.make_sweeps(np.tile(f32([1.0, 0.5, -4.0]), (BAD, 1)), np.tile(f32([0.0, 0.3, 1.0]), (BAD, 1)), f32(0.25), f32(50.0))
    bad["direction"][0] = 0.0
    bad["direction"][1, 1] = nan
    bad["origin"][2, 0] = nan
    bad["origin"][3, 2] = inf
    bad["t_max"][4], bad["t_max"][5], bad["t_max"][6] = -1.0, inf, nan
    bad["radius"][7], bad["radius"][8] = -0.5, inf
    return np.concatenate([rec, bad])


# -- 2. several pinned instances -------------------------------------------------------------------------------------------------------
def pinned_instances_scene():
    """Translations by fp32 numbers, scales that are powers of two, no rotation: every rounding is pinned.  Index 3 duplicates index 1."""
    a = volume(3, EXTENT, sphere_fn(0.6 * EXTENT), _abi.FORMAT_F32)
    b = volume(2, 2.0, None, _abi.FORMAT_TEXEL16, random_field(5, 7))
    twin = dict(Position=(8.0, 0.5, -0.25), Scale=(2.0, 2.0, 2.0), Volume=a)
    objs = [v.VVoxelObject(Volume=a), v.VVoxelObject(**twin), v.VVoxelObject(Position=(-6.5, 1.0, 2.0), Scale=(0.5, 0.5, 0.5), Volume=b),
            v.VVoxelObject(**twin), v.VVoxelObject(Position=(0.0, 9.0, 0.0), Scale=(2.0, 0.5, 1.0), Volume=b)]
    return v.VScene(Objects=objs)


def pinned_instances_records(seed=23, n=2500):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-16.0, 16.0, (n, 3))
    d = unit(rng, n) * rng.uniform(0.5, 2.0, (n, 1))
    d[::2] = (rng.uniform(-9.0, 9.0, (len(d[::2]), 3)) - o[::2])  # every other one aims at the middle of the scene
    radius = rng.choice([0.0, 0.4, 1.1], n)
    t_max = rng.uniform(3.0, 40.0, n)
    return v.make_sweeps(o, d, radius, t_max)


# -- 3. one placed instance ------------------------------------------------------------------------------------------------------------
def placed_one_scene():
    vol = volume(3, EXTENT, sphere_fn(0.6 * EXTENT), _abi.FORMAT_F32)
    vol.material_id = np.random.default_rng(5).integers(0, 256, vol.material_id.shape).astype(np.uint8)
    q = tuple(float(x) for x in v.quat_from_axis_angle((1.0, -2.0, 0.5), 0.9))
    return v.VScene(Objects=[v.VVoxelObject(Position=(0.7, -0.4, 0.3), Rotation=q, Scale=(1.0, -0.8, 1.3), Volume=vol)])


def placed_one_records(seed=33, n=2500):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-9.0, 9.0, (n, 3))
    d = rng.uniform(-2.5, 2.5, (n, 3)) - o
    d[::4] = unit(rng, len(d[::4]))
    radius = rng.choice([0.0, 0.3, 0.8], n)
    t_max = rng.uniform(2.0, 30.0, n)
    return v.make_sweeps(o, d, radius, t_max)


# -- 4. four placed instances ----------------------------------------------------------------------------------------------------------
PLACED_STEPS, PLACED_TOLERANCE, PLACED_STEP_MIN = 256, 0.02, 0.05
# The largest difference between sweep_ref in fp32 and in fp64 on placed_records(), over the records that fp64 decides by more than
# PLACED_MARGIN: measured by test_query_sweeps.py, which asserts that it stays below this figure (reference against reference).
PLACED_REF_DIFFERENCE = 5e-6  # measured: 4.43e-6
PLACED_FACTOR = 4.0   # the library packs its matrices in another operation order than points_ref.pack_w2o
PLACED_MARGIN = PLACED_REF_DIFFERENCE * PLACED_FACTOR
AMBIGUOUS_CAP = 0.05


def placed_scene():
    a = volume(3, 3.3, sphere_fn(2.1), _abi.FORMAT_F32)
    box = lambda X, Y, Z: (np.maximum(np.maximum(np.abs(X) - f32(1.6), np.abs(Y) - f32(1.1)), np.abs(Z) - f32(2.0))).astype(f32)
    b = volume(4, 2.9, box, _abi.FORMAT_TEXEL16)
    b.material_id = np.random.default_rng(3).integers(0, 256, b.material_id.shape).astype(np.uint8)
    q1 = tuple(float(x) for x in v.quat_from_axis_angle((1.0, 2.0, 3.0), 0.7))
    q2 = tuple(float(x) for x in v.quat_from_axis_angle((-2.0, 0.5, 1.0), 2.1))
    q3 = tuple(float(x) for x in v.quat_from_axis_angle((0.3, -1.0, 0.2), 1.3))
    first = dict(Position=(0.4, -0.3, 0.2), Rotation=q1, Scale=(1.0, 0.8, 1.3), Volume=a)
    objs = [v.VVoxelObject(**first), v.VVoxelObject(Position=(5.9, 0.8, -0.6), Rotation=q2, Scale=(0.7, 1.2, 0.9), Volume=b),
            v.VVoxelObject(Position=(-3.5, 4.0, 2.1), Rotation=q3, Scale=(1.4, -0.9, 0.75), Volume=a), v.VVoxelObject(**first)]
    return v.VScene(Objects=objs)


def placed_records(seed=43, n=3000):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-11.0, 11.0, (n, 3))
    d = rng.uniform(-5.0, 6.0, (n, 3)) - o
    d[::5] = unit(rng, len(d[::5]))
    radius = rng.choice([0.0, 0.2, 0.5], n)
    t_max = rng.uniform(4.0, 30.0, n)
    return v.make_sweeps(o, d, radius, t_max)


# -- 5. capacity -----------------------------------------------------------------------------------------------------------------------
LATTICE_STEPS, LATTICE_TOLERANCE, LATTICE_STEP_MIN = 128, 0.1, 0.25
LATTICE_MARGIN = 2e-4  # test_query_points_gpu's figure for this scene, see there


def lattice_records(seed=53, n=1500):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-190.0, 190.0, (n, 3))
    d = rng.uniform(-150.0, 150.0, (n, 3)) - o
    radius = rng.choice([0.0, 1.0, 3.0], n)
    t_max = rng.uniform(20.0, 400.0, n)
    t_max[::3] = rng.uniform(5.0, 60.0, len(t_max[::3]))
    return v.make_sweeps(o, d, radius, t_max)


# -- the analytic spheres of test_query_points.py, cells of 1 --------------------------------------------------------------------------
SPHERES = {9: 2.6, 17: 5.2}   # N: radius in cells
SPHERE_TOLERANCE, SPHERE_STEP_MIN, SPHERE_STEPS = 1e-3, 1e-3, 128


def sphere_slot(N: int) -> P.Slot:
    extent = 0.5 * (N - 1)
    a = np.arange(N, dtype=f32) - f32(extent)
    X, Z, Y = a[:, None, None], a[None, :, None], a[None, None, :]
    d = (np.sqrt((X * X + Y * Y) + Z * Z) - f32(SPHERES[N])).astype(f32)
    return P.Slot(stored=d, material=(d <= 0).astype(np.uint8), fmt=P.F32, extent=extent)


def sphere_records(N, radius, n=3000, seed=11):
    """Seeded sweeps from a shell around the box, aimed at a disc a little larger than the sphere grown by the radius."""
    extent = 0.5 * (N - 1)
    rng = np.random.default_rng(seed + N + int(radius * 8))
    o = unit(rng, n) * rng.uniform(1.8 * extent, 2.6 * extent, (n, 1))
    aim = unit(rng, n) * (SPHERES[N] + radius + 0.6) * np.sqrt(rng.uniform(0, 1, (n, 1)))
    return v.make_sweeps(o, aim - o, radius, 10.0 * extent)
