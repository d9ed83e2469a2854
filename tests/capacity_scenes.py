"""Seeded scenes at the limits include/vrt.h promises (VRT_MAX_INSTANCES 64, VRT_MAX_VOLUMES 20, VRT_MAX_POINT_LIGHTS 5,
VRT_MAX_SPOT_LIGHTS 5) and scenes that corner the instance BVH: exact ties, equal centres, a row seen end-on, odd boxes.
test_scene_capacity.py states on the CPU oracle alone what each scene has to contain; test_scene_capacity_gpu.py renders them.
Every builder is deterministic and memoised: the tests share one object per scene and never write to it (copy first).
No GPU and no oracle here."""
import copy
import math

import numpy as np

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

W, H = 96, 54
LATTICE_FORMATS = ("f32", "texel16", "mixed")
_cache = {}


def _memo(fn):
    def wrapped(*args):
        key = (fn.__name__,) + args
        if key not in _cache:
            _cache[key] = fn(*args)
        return _cache[key]

    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def look_at(position, target, fov=60.0, roll=0.0) -> v.VCamera:
    """A camera at `position` whose forward axis (+X turned by its rotation) points at `target`, rolled about it by `roll`."""
    dx, dy, dz = (float(p) - float(t) for p, t in zip(position, target))
    yaw, pitch = math.atan2(-dy, -dx), math.atan2(dz, math.hypot(dx, dy))
    q = v.quat_mul(v.quat_mul(v.quat_from_axis_angle(v.UP, yaw), v.quat_from_axis_angle(v.RIGHT, pitch)), v.quat_from_axis_angle(v.FORWARD, roll))
    return v.VCamera(Position=tuple(float(x) for x in position), Rotation=tuple(float(x) for x in q), FOVAngle=float(fov))


def with_camera(sc: v.VScene, cam: v.VCamera) -> v.VScene:
    out = copy.copy(sc)
    out.Camera = cam
    return out


def params(sc: v.VScene, mode=_abi.MODE_INTERP_NOTEX, path=_abi.PATH_AUTO, flags=0, bounces=0, w=W, h=H) -> _abi.vrt_params:
    """The suite's march contract for a frame of `sc` (the cell of its finest volume, 255 positions, shadows on)."""
    p = v.default_params(w, h, min(vol.GetCellSize() for vol in sc.volumes()), 255, shadow=True, mode=mode, path=path)
    p.max_bounces = int(bounces)
    p.flags |= int(flags)
    return p


def _sky():
    if "sky" not in _cache:
        _cache["sky"] = v.procedural_skybox(16)
    return _cache["sky"]


def _spot(position, target, strength, color, angle=40.0, falloff=25.0):
    cam = look_at(position, target)  # (the same forward axis: +X turned by the rotation)
    return v.VSpotLight(Position=cam.Position, Rotation=cam.Rotation, IlluminationStrength=float(strength), Color=tuple(color) + (1.0,),
                        AttenuationLinear=0.01, AttenuationExp=0.0002, FalloffAngle=float(falloff), Angle=float(angle))


def _point(position, strength, color):
    return v.VPointLight(Position=tuple(float(x) for x in position), IlluminationStrength=float(strength), Color=tuple(color) + (1.0,),
                         AttenuationLinear=0.02, AttenuationExp=0.001)


# ---- 1. the lattice: every limit at once --------------------------------------------------------------------------------------

LATTICE_PITCH = 70.0


def _lattice_volumes():
    """20 distinct volumes: spheres and tori at resolutions 3 and 4, one at 5; every fourth material is smooth enough to mirror."""
    rng = np.random.default_rng(6420)
    vols = []
    for k in range(_abi.VRT_MAX_VOLUMES):
        res = 5 if k == 7 else 3 + (k % 2)
        rough = 0.15 if k % 4 == 1 else float(rng.uniform(0.4, 0.9))
        mat = v.VMaterial(tuple(float(c) for c in rng.uniform(0.15, 1.0, 3)) + (1.0,), rough, float(rng.uniform(0.0, 0.7)))
        if k % 3 == 2:
            vols.append(v.torus_volume(res, 100.0, float(rng.uniform(50, 58)), float(rng.uniform(24, 30)), mat))
        else:
            vols.append(v.sphere_volume(res, 100.0, float(rng.uniform(55, 80)), mat))
    return vols


@_memo
def lattice64(fmt="f32") -> v.VScene:
    """64 instances of 20 volumes on a 4x4x4 lattice (pitch 70, scale about 0.3: boxes of 60 with gaps of 10), seeded rotations, a
    quarter of them scaled anisotropically, every seventh mirrored; 5 point lights between the lattice planes, 5 spot lights around
    it, the directional light, a sky.  fmt: "f32", "texel16" or "mixed" (formats alternate by volume)."""
    assert fmt in LATTICE_FORMATS
    rng = np.random.default_rng(64)
    vols = _lattice_volumes()
    for k, vol in enumerate(vols):
        f16 = fmt == "texel16" or (fmt == "mixed" and k % 2 == 1)
        vol.set_device_format(_abi.FORMAT_TEXEL16 if f16 else _abi.FORMAT_F32)
    objs = []
    for k in range(_abi.VRT_MAX_INSTANCES):
        ix, iy, iz = k % 4, (k // 4) % 4, k // 16
        axis = rng.normal(size=3)
        q = v.quat_from_axis_angle(tuple(axis / np.linalg.norm(axis)), float(rng.uniform(0, 2 * math.pi)))
        s = np.full(3, float(rng.uniform(0.27, 0.33)))
        if k % 4 == 3:
            s = s * rng.uniform(0.7, 1.0, 3)
        if k % 7 == 5:
            s[int(rng.integers(0, 3))] *= -1.0
        objs.append(v.VVoxelObject(Position=((ix - 1.5) * LATTICE_PITCH, (iy - 1.5) * LATTICE_PITCH, (iz - 1.5) * LATTICE_PITCH), Rotation=tuple(float(x) for x in q),
                                   Scale=tuple(float(x) for x in s), Volume=vols[(k * 7 + k // 20) % len(vols)]))
    g = LATTICE_PITCH
    colors = [(1.0, 0.5, 0.4), (0.4, 1.0, 0.5), (0.5, 0.5, 1.0), (1.0, 1.0, 0.4), (0.4, 1.0, 1.0)]
    # between the lattice planes, towards the camera's side: each lights the faces around it and is shadowed by its neighbours
    points = [_point(pos, 260.0, colors[k]) for k, pos in enumerate([(g, 0.0, 0.0), (2.2 * g, g, g), (2.2 * g, -g, -g), (0.0, -2.3 * g, g), (0.0, g, 2.3 * g)])]
    spots = [_spot(pos, tgt, 2600.0, colors[(k + 2) % 5], angle=28.0, falloff=18.0) for k, (pos, tgt) in enumerate([
        ((420.0, 160.0, 200.0), (105.0, 105.0, 105.0)), ((420.0, -160.0, 200.0), (105.0, -105.0, 105.0)),
        ((420.0, 160.0, -120.0), (105.0, 105.0, -105.0)), ((420.0, -160.0, -120.0), (105.0, -105.0, -105.0)),
        ((300.0, 0.0, 420.0), (35.0, 0.0, 105.0))])]
    return v.VScene(Camera=look_at((430.0, 95.0, 215.0), (0.0, 0.0, -10.0), 50.0), DirectionalLight=v.demo_light(), Objects=objs, PointLights=points,
                    SpotLights=spots, EnvironmentMap=_sky())


# ---- 2. coincident instances: exact ties -------------------------------------------------------------------------------------

RED, GREEN = (1.0, 0.05, 0.05, 1.0), (0.05, 1.0, 0.05, 1.0)


@_memo
def coincident(order=0, variant="two_volumes", fmt=_abi.FORMAT_F32) -> v.VScene:
    """Instances that coincide exactly, so every camera ray that hits one hits its twin at the same t.
    two_volumes: two volumes with the same field, one red and one green, placed with the same transform at indices 1 and 3; indices
    0 and 2 are far away on either side, so the BVH's preorder (2, 1, 3, 0) is not index order.  order = 0: red has the lower index.
    same_slot: the red volume twice (the twin is told from its index alone).  pairs32: 32 coincident pairs on a 4x4x2 lattice,
    pair j at indices j and 63 - j.
    shifted: twins whose BOXES differ, so that the walk meets the higher index first (equal boxes always sort lower index first):
    cells of 8 and a scale of 2 (powers of two), the higher twin's volume holds the same sphere two cells off centre and stands two
    cells back, so the solid voxels coincide in the world and a Cube mode's entry planes are hit at bit-equal t; the fillers stand
    along x, which makes the preorder (2, 3, 1, 0).  (A sphere-trace starts at each box's own entry: there the twins merely agree.)"""
    if variant == "shifted":
        vols = []
        for centre, color in zip(((0.0, 0.0, 0.0), (16.0, 0.0, 0.0)), (RED, GREEN) if order == 0 else (GREEN, RED)):
            vol = v.VVoxelVolume(4, 64.0)
            gen = v.VDensityGenerator()
            gen.GetRootShape().AddChild(v.VSphere(30.0, position=centre))
            vol.fill(gen.Evaluate)
            vol.Material = v.VMaterial(color, 0.8, 0.0)
            vols.append(vol.set_device_format(fmt))
        objs = [v.VVoxelObject(Position=(4000.0, 0.0, 0.0), Volume=vols[0]), v.VVoxelObject(Position=(0.0, 8.0, 8.0), Scale=(2.0, 2.0, 2.0), Volume=vols[0]),
                v.VVoxelObject(Position=(-4000.0, 0.0, 0.0), Volume=vols[1]), v.VVoxelObject(Position=(-32.0, 8.0, 8.0), Scale=(2.0, 2.0, 2.0), Volume=vols[1])]
        return v.VScene(Camera=v.look_minus_x_camera(330.0, 20.0), DirectionalLight=v.demo_light(), Objects=objs, EnvironmentMap=_sky())
    a = v.sphere_volume(4, 100.0, 70.0, v.VMaterial(RED, 0.8, 0.0)).set_device_format(fmt)
    b = v.sphere_volume(4, 100.0, 70.0, v.VMaterial(GREEN, 0.8, 0.0)).set_device_format(fmt)
    first, second = (a, b) if order == 0 else (b, a)
    rot = tuple(float(x) for x in v.quat_from_axis_angle((1.0, 2.0, 3.0), 0.7))
    if variant == "pairs32":
        rng = np.random.default_rng(32)
        objs = [None] * 64
        for j in range(32):
            pos = ((j % 4 - 1.5) * 90.0, ((j // 4) % 4 - 1.5) * 90.0, (j // 16 - 0.5) * 90.0)
            axis = rng.normal(size=3)
            q = tuple(float(x) for x in v.quat_from_axis_angle(tuple(axis / np.linalg.norm(axis)), float(rng.uniform(0, 6.28))))
            s = tuple(float(x) for x in rng.uniform(0.3, 0.42, 3))
            objs[j] = v.VVoxelObject(Position=pos, Rotation=q, Scale=s, Volume=first)
            objs[63 - j] = v.VVoxelObject(Position=pos, Rotation=q, Scale=s, Volume=second)
        return v.VScene(Camera=look_at((520.0, 130.0, 330.0), (0.0, 0.0, 0.0), 48.0), DirectionalLight=v.demo_light(), Objects=objs, EnvironmentMap=_sky())
    if variant == "same_slot":
        second = first
    else:
        assert variant == "two_volumes"
    twin = dict(Position=(0.0, 10.0, 5.0), Rotation=rot, Scale=(1.0, 0.8, 1.2))
    objs = [v.VVoxelObject(Position=(0.0, 4000.0, 0.0), Volume=first), v.VVoxelObject(Volume=first, **twin),
            v.VVoxelObject(Position=(0.0, -4000.0, 0.0), Volume=second), v.VVoxelObject(Volume=second, **twin)]
    return v.VScene(Camera=v.look_minus_x_camera(330.0, 20.0), DirectionalLight=v.demo_light(), Objects=objs, EnvironmentMap=_sky())


# ---- 3. 64 concentric instances: every BVH split ties ------------------------------------------------------------------------

NESTED_CAMERAS = ("outside", "inside")


@_memo
def nested64(camera="outside") -> v.VScene:
    """64 concentric instances of one sphere volume (radius 40 in a box of 100), scales 0.3 .. 1.8 in a seeded order: all centres are
    equal, so every median split falls to the index rule and no box can be culled.  Cameras: outside all of them; inside every box
    (|x| < 30) but outside the smallest sphere (radius 12)."""
    assert camera in NESTED_CAMERAS
    vol = v.sphere_volume(4, 100.0, 40.0, v.VMaterial((0.9, 0.7, 0.3, 1.0), 0.7, 0.1))
    scales = np.linspace(0.3, 1.8, 64)[np.random.default_rng(3).permutation(64)]
    objs = [v.VVoxelObject(Position=(5.0, -3.0, 2.0), Scale=(float(s),) * 3, Volume=vol) for s in scales]
    cam = look_at((250.0, 40.0, 60.0), (5.0, -3.0, 2.0), 55.0) if camera == "outside" else look_at((25.0, -3.0, 2.0), (5.0, -3.0, 2.0), 70.0)
    return v.VScene(Camera=cam, DirectionalLight=v.demo_light(), Objects=objs, EnvironmentMap=_sky())


# ---- 4. 64 instances in a row -----------------------------------------------------------------------------------------------

LINE_VIEWS = ("along", "back", "diagonal")
LINE_PITCH = 30.0


def line_centre(axis: int, k: int):
    c = [0.0, 0.0, 0.0]
    c[axis] = (k - 31.5) * LINE_PITCH
    return tuple(c)


@_memo
def line64(axis=0, view="along") -> v.VScene:
    """64 instances of one sphere volume in a row along world axis `axis` (pitch 30), each squeezed to a disc across the row (boxes 10
    thick and 30 to 60 wide), shifted sideways by up to 10 and placed in a seeded index order, so that the first disc a ray meets is
    now an early, now a late one.  along: seen from the row's low end, a little off its axis: the central rays pierce all 64 boxes
    and the closest hit so far prunes from front to back; back: from the other end; diagonal: from the side, rolled so the row runs
    along a screen diagonal and each wave meets few boxes."""
    assert view in LINE_VIEWS
    vol = v.sphere_volume(3, 100.0, 60.0, v.VMaterial((0.4, 0.7, 0.95, 1.0), 0.6, 0.2))
    rng = np.random.default_rng(11)
    order = rng.permutation(64)
    side = [(axis + 1) % 3, (axis + 2) % 3]
    objs = [None] * 64
    for k in range(64):
        pos, s = list(line_centre(axis, k)), [0.0, 0.0, 0.0]
        pos[side[0]], pos[side[1]] = float(rng.uniform(-10, 10)), float(rng.uniform(-10, 10))
        s[axis], s[side[0]], s[side[1]] = 0.05, float(rng.uniform(0.15, 0.3)), float(rng.uniform(0.15, 0.3))
        objs[int(order[k])] = v.VVoxelObject(Position=tuple(pos), Scale=tuple(s), Volume=vol)
    end = 32.0 * LINE_PITCH + 100.0
    pos, tgt = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    if view == "diagonal":
        pos[axis], pos[side[0]], pos[side[1]] = -250.0, 200.0, 80.0
        tgt[axis] = -50.0
        cam = look_at(pos, tgt, 46.0, roll=math.radians(42.0))
    else:
        sign = -1.0 if view == "along" else 1.0
        pos[axis], pos[side[0]], pos[side[1]] = sign * end, 2.0, 1.0
        tgt[axis] = -sign * end
        cam = look_at(pos, tgt, 8.0)
    return v.VScene(Camera=cam, DirectionalLight=v.demo_light(), Objects=objs, EnvironmentMap=_sky())


# ---- 5. odd boxes -------------------------------------------------------------------------------------------------------------

ODD_CAMERAS = ("near", "far")
FAR_X = 1.0e5


@_memo
def odd_boxes(camera="near") -> v.VScene:
    """0: a box volume squeezed to 1e-3 along z (a flat box); 1: a sphere at (1e5, 0, 0), where the box's relative pad is 10 units;
    2: a box turned 45 degrees about two axes (the widest world box of a cube); 3: a torus at the origin.  near: the three around the
    origin; far: the camera beside the distant sphere."""
    assert camera in ODD_CAMERAS
    box = v.VVoxelVolume(4, 100.0)
    gen = v.VDensityGenerator()
    gen.GetRootShape().AddChild(v.VBox((70.0, 70.0, 70.0)))
    box.fill(gen.Evaluate)
    box.Material = v.VMaterial((0.8, 0.8, 0.3, 1.0), 0.7, 0.0)
    ball = v.sphere_volume(4, 100.0, 70.0, v.VMaterial((0.9, 0.3, 0.3, 1.0), 0.6, 0.1))
    torus = v.torus_volume(4, 100.0, 55.0, 25.0, v.VMaterial((0.3, 0.6, 0.9, 1.0), 0.6, 0.1))
    q45 = v.quat_mul(v.quat_from_axis_angle(v.UP, math.radians(45.0)), v.quat_from_axis_angle(v.RIGHT, math.radians(45.0)))
    objs = [v.VVoxelObject(Position=(0.0, -150.0, -60.0), Scale=(1.0, 1.0, 1e-3), Volume=box),
            v.VVoxelObject(Position=(FAR_X, 0.0, 0.0), Scale=(0.5, 0.5, 0.5), Volume=ball),
            v.VVoxelObject(Position=(-40.0, 170.0, 20.0), Rotation=tuple(float(x) for x in q45), Scale=(0.7, 0.7, 0.7), Volume=box),
            v.VVoxelObject(Position=(0.0, 0.0, 0.0), Rotation=tuple(float(x) for x in v.quat_from_axis_angle(v.RIGHT, 0.5)), Volume=torus)]
    cam = look_at((420.0, 0.0, 150.0), (0.0, 0.0, -10.0), 60.0) if camera == "near" else look_at((FAR_X + 15.0, 120.0, 30.0), (FAR_X, 0.0, 0.0), 50.0)
    return v.VScene(Camera=cam, DirectionalLight=v.demo_light(), Objects=objs, EnvironmentMap=_sky())


# ---- 6. lights ----------------------------------------------------------------------------------------------------------------

LIGHT_CASES = ((5, 5), (5, 0), (0, 5), (1, 5))


@_memo
def lights(n_point=5, n_spot=5) -> v.VScene:
    """A tilted torus over a ground slab (2 instances) under a ring of point lights and a wider ring of spot lights: each light casts
    the torus' shadow onto a part of the slab of its own.  Counts above five are light OBJECTS: the first five of lights(7, 7) are
    the lights of lights(5, 5)."""
    slab = v.VVoxelVolume(3, 100.0)
    gen = v.VDensityGenerator()
    gen.GetRootShape().AddChild(v.VBox((85.0, 85.0, 40.0)))
    slab.fill(gen.Evaluate)
    slab.Material = v.VMaterial((0.8, 0.8, 0.8, 1.0), 0.9, 0.0)
    torus = v.torus_volume(4, 100.0, 55.0, 24.0, v.VMaterial((0.9, 0.6, 0.2, 1.0), 0.6, 0.1))
    objs = [v.VVoxelObject(Position=(0.0, 0.0, 40.0), Rotation=tuple(float(x) for x in v.quat_from_axis_angle(v.RIGHT, 0.35)), Scale=(0.8, 0.8, 0.8), Volume=torus),
            v.VVoxelObject(Position=(0.0, 0.0, -60.0), Scale=(3.2, 3.2, 0.5), Volume=slab)]
    colors = [(1.0, 0.4, 0.3), (0.3, 1.0, 0.4), (0.4, 0.4, 1.0), (1.0, 1.0, 0.3), (0.3, 1.0, 1.0), (1.0, 0.3, 1.0), (1.0, 1.0, 1.0)]
    points, spots = [], []
    for k in range(7):
        a = math.radians(72.0 * k + (0.0 if k < 5 else 36.0))
        points.append(_point((150.0 * math.cos(a), 150.0 * math.sin(a), 150.0), 160.0, colors[k]))
        b = math.radians(72.0 * k + 36.0 + (0.0 if k < 5 else 36.0))
        spots.append(_spot((260.0 * math.cos(b), 260.0 * math.sin(b), 230.0), (-60.0 * math.cos(b), -60.0 * math.sin(b), -40.0), 1500.0, colors[6 - k], angle=50.0, falloff=30.0))
    light = v.VLight(Rotation=v.demo_light().Rotation, IlluminationStrength=2.0)
    return v.VScene(Camera=look_at((420.0, 60.0, 330.0), (0.0, 0.0, -20.0), 58.0), DirectionalLight=light, Objects=objs,
                    PointLights=points[:n_point], SpotLights=spots[:n_spot], EnvironmentMap=_sky())


def without_light(sc: v.VScene, k: int) -> v.VScene:
    """`sc` without its k-th light (point lights first, then spot lights)."""
    out = copy.copy(sc)
    n = len(sc.PointLights)
    if k < n:
        out.PointLights = sc.PointLights[:k] + sc.PointLights[k + 1:]
    else:
        out.SpotLights = sc.SpotLights[:k - n] + sc.SpotLights[k - n + 1:]
    return out


# ---- instance boxes, as the host builds them ---------------------------------------------------------------------------------

def instance_boxes(sc: v.VScene, dtype=np.float32):
    """World boxes (lo [n, 3], hi [n, 3]) of the scene's instances as instance_box (csrc/vrt_render.hip) builds them — the eight
    corners of the volume box through o2w = scale_i * R_ij, min / max, then a pad of 1e-4 * (1 + max |bound|) — in `dtype`:
    float32 restates the host's arithmetic, operation by operation; float64 is the plain box for counting what a ray meets."""
    f = dtype
    lo, hi = [], []
    for o in sc.Objects:
        x, y, z, w = (f(c) for c in o.Rotation)
        one, two = f(1.0), f(2.0)
        R = [[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
             [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
             [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]]
        e = f(o.Volume.VolumeExtends)
        blo, bhi = [f(np.inf)] * 3, [f(-np.inf)] * 3
        for k in range(8):
            c = [e if k & 1 else -e, e if k & 2 else -e, e if k & 4 else -e]
            for a in range(3):
                m = [f(o.Scale[a]) * R[a][j] for j in range(3)]
                wv = m[0] * c[0] + m[1] * c[1] + m[2] * c[2] + f(o.Position[a])
                blo[a], bhi[a] = min(blo[a], wv), max(bhi[a], wv)
        for a in range(3):
            pad = f(1e-4) * (one + max(abs(blo[a]), abs(bhi[a])))
            blo[a], bhi[a] = blo[a] - pad, bhi[a] + pad
        lo.append(blo)
        hi.append(bhi)
    return np.array(lo, dtype), np.array(hi, dtype)
