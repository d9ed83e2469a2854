"""Plain-numpy restatement of the rule by which a hit on a slot with a palette gets its entry (include/vrt.h, vrt_volume_set_palette),
written from the header rather than from the kernel, and the painted sphere the palette tests render.

entry_ids() takes a downloaded volume (decoded densities and material ids, both [x, z, y]) and object-space hit points and returns, per
point, the material id the rule picks and the point's distance, in cells, to the nearest place where the rule's decision changes: a cell
face (the cell c changes), the bisector plane of the best INSIDE corner and any other INSIDE corner (the chosen corner changes — the two
best corners' bisector among them) or, in a cell without an INSIDE corner, a half-cell plane of the nearest-sample rule.  The device
computes the hit point in fp32 with its own rounding; a test compares only where that distance exceeds a margin far above fp32 rounding.
Every operation on g, c and f is an np.float32 operation in the header's parenthesisation."""
from __future__ import annotations

import math

import numpy as np

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

f32 = np.float32
MARGIN_CELLS = 1e-3   # hit pixels nearer than this to a decision boundary are excluded from bit-for-bit comparisons
EXCLUDED_CAP = 0.02   # ... and must stay below this share of the hit pixels


def object_points(position, rotation, scale, origins, directions, t) -> np.ndarray:
    """Object-space hit points p = w2o (o - pos) + (w2o d) t with w2o = R^T S^-1 (float64 here; the device: fp32 with one fma)."""
    o = (np.asarray(origins, np.float64).reshape(-1, 3) - np.asarray(position, np.float64)) / np.asarray(scale, np.float64)
    d = np.asarray(directions, np.float64).reshape(-1, 3) / np.asarray(scale, np.float64)
    qi = v.quat_inverse(rotation)
    oo = np.stack([v.quat_rotate(qi, x) for x in o]).astype(np.float64)
    od = np.stack([v.quat_rotate(qi, x) for x in d]).astype(np.float64)
    return oo + od * np.asarray(t, np.float64).reshape(-1, 1)


def entry_ids(density: np.ndarray, material: np.ndarray, extent: float, points_xyz):
    """(ids [n] int, boundary distance in cells [n] float64) of the object-space points; density: the DECODED densities [x, z, y] (a
    VRT_FORMAT_TEXEL16 slot's q * 0.01f keeps the stored field's sign, -0.0 included), material: uint8 [x, z, y]."""
    N = density.shape[0]
    cell = f32(f32(extent) * f32(2.0)) / f32(N - 1)
    inv_cell = f32(1.0) / cell
    p = np.asarray(points_xyz, np.float64).reshape(-1, 3).astype(f32)
    n = len(p)
    g = ((p + f32(extent)) * inv_cell).astype(f32)                       # g_a = (p_a + extent) * inv_cell
    c = np.clip(np.floor(g), f32(0), f32(N - 2)).astype(np.int64)        # c_a = clamp(floor(g_a), 0, N-2)
    f = (g - c.astype(f32)).astype(f32)                                  # f_a = g_a - (float)c_a
    d2 = np.zeros((n, 8), f32)
    inside = np.zeros((n, 8), bool)
    corner = np.zeros((8, 3), np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(8):
            dx, dy, dz = j & 1, (j >> 1) & 1, j >> 2
            corner[j] = (dx, dy, dz)
            d = density[c[:, 0] + dx, c[:, 2] + dz, c[:, 1] + dy]
            inside[:, j] = ~np.isnan(d) & (d <= f32(0))
            ex, ey, ez = f[:, 0] - f32(dx), f[:, 1] - f32(dy), f[:, 2] - f32(dz)
            d2[:, j] = (ex * ex + ey * ey) + ez * ez
    key = np.where(inside, d2, f32(np.inf))
    best = np.argmin(key, axis=1)                                        # the first (lowest j) of equal minima
    any_inside = inside.any(axis=1)
    near = np.clip(np.floor(g + f32(0.5)), f32(0), f32(N - 1)).astype(np.int64)  # vrt_hit::voxel's sample
    chosen = np.where(any_inside[:, None], c + corner[best], near)
    ids = material[chosen[:, 0], chosen[:, 2], chosen[:, 1]].astype(np.int64)
    # distance to the nearest decision boundary, in cells (float64 from the fp32 f)
    F = f.astype(np.float64)
    dist = np.minimum(F, 1.0 - F).min(axis=1)                            # cell faces
    half = np.abs(F - 0.5).min(axis=1)                                   # nearest-sample planes
    D2 = d2.astype(np.float64)
    bis = np.full(n, np.inf)
    for j in range(8):
        sep = np.linalg.norm((corner[j][None, :] - corner[best]).astype(np.float64), axis=1)
        other = inside[:, j] & (sep > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            dj = (D2[:, j] - D2[np.arange(n), best]) / (2.0 * sep)
        bis = np.where(other, np.minimum(bis, dj), bis)
    dist = np.where(any_inside, np.minimum(dist, bis), np.minimum(dist, half))
    return ids, dist


# ---- the scene the palette tests render --------------------------------------------------------------------------------------------
RESOLUTION, EXTENT, RADIUS_CELLS, PAINT_X = 5, 16.0, 10.4, 16.3   # N = 33, cells of 1.0: a sphere of 10.4 cells, id 2 where x > 16.3
WIDTH, HEIGHT = 96, 54
ENTRIES = (((0.8, 0.8, 0.8, 1.0), 0.8, 0.0), ((0.9, 0.2, 0.1, 1.0), 0.5, 0.1), ((0.1, 0.3, 0.9, 1.0), 0.35, 0.6))  # all rough: no bounce


def sphere_volume(fmt: int = _abi.FORMAT_F32) -> v.VVoxelVolume:
    """The sphere SDF, ids 1 inside and 0 outside (material = density <= 0), not painted yet."""
    vol = v.VVoxelVolume(RESOLUTION, EXTENT)
    vol.fill(lambda X, Y, Z: np.sqrt((X * X + Y * Y) + Z * Z).astype(f32) - f32(RADIUS_CELLS))
    vol.set_device_format(fmt)
    return vol


# The mirror stands beside the sphere, turned so that the camera sees the sphere's image in it; for the mirror test the sphere is turned
# further (MIRROR_SPHERE_YAW), so that both painted halves face the mirror as well as the camera.
MIRROR_AT, MIRROR_YAW_DEG, MIRROR_SPHERE_YAW = (-24.0, -6.0, 0.0), 35.0, 1.2


def mirror_volume() -> v.VVoxelVolume:
    """A slab (thin along its own x) of roughness 0.1: it mirrors.  No palette."""
    vol = v.VVoxelVolume(RESOLUTION, EXTENT)
    h = (f32(1.5), f32(14.0), f32(14.0))

    def box(X, Y, Z):
        qx, qy, qz = np.abs(X) - h[0], np.abs(Y) - h[1], np.abs(Z) - h[2]
        out = np.sqrt((np.maximum(qx, 0) ** 2 + np.maximum(qy, 0) ** 2) + np.maximum(qz, 0) ** 2)
        return (out + np.minimum(np.maximum(qx, np.maximum(qy, qz)), 0)).astype(f32)

    vol.fill(box)
    vol.Material = v.VMaterial((0.9, 0.9, 0.9, 1.0), 0.1, 0.8)
    return vol


def paint_record() -> _abi.vrt_brush:
    """The PAINT box that gives id 2 to the inside samples with x > PAINT_X."""
    N = (1 << RESOLUTION) + 1
    hx = 0.5 * (N + 4 - PAINT_X)
    return v.box_brush(_abi.BRUSH_PAINT, (PAINT_X + hx, 0.5 * (N - 1), 0.5 * (N - 1)), (hx, float(N), float(N)), material=2)


def painted_sphere_scene(vol: v.VVoxelVolume, mirror: v.VVoxelVolume = None, yaw: float = 0.35) -> v.VScene:
    """The sphere, turned and stretched so that the instance transform matters, seen from +Y so that both halves show; one directional
    and one spot light.  mirror: a second volume placed beside the sphere (MIRROR_AT)."""
    objs = [v.VVoxelObject(Position=(1.0, 0.0, -0.5), Rotation=tuple(v.quat_from_axis_angle(v.UP, yaw)), Scale=(1.1, 1.0, 0.9), Volume=vol)]
    if mirror is not None:
        objs.append(v.VVoxelObject(Position=MIRROR_AT, Rotation=tuple(v.quat_from_axis_angle(v.UP, math.radians(MIRROR_YAW_DEG))), Volume=mirror))
    cam = v.VCamera(Position=(2.0, 34.0, 6.0), Rotation=tuple(v.quat_mul(v.quat_from_axis_angle(v.UP, math.radians(-90.0)),
                                                                      v.quat_from_axis_angle(v.RIGHT, math.radians(10.0)))), FOVAngle=60.0)
    spot_dir = v.quat_mul(v.quat_from_axis_angle(v.UP, math.radians(-60.0)), v.quat_from_axis_angle(v.RIGHT, math.radians(25.0)))
    spot = v.VSpotLight(Position=(-14.0, 26.0, 14.0), Rotation=tuple(spot_dir), IlluminationStrength=60.0, Color=(1.0, 0.9, 0.6, 1.0),
                        AttenuationLinear=0.02, AttenuationExp=0.001, FalloffAngle=25.0, Angle=70.0)
    return v.VScene(Camera=cam, DirectionalLight=v.demo_light(), Objects=objs, SpotLights=[spot], EnvironmentMap=v.procedural_skybox(16))


def scene_params(sc: v.VScene, mode: int = _abi.MODE_INTERP_NOTEX, path: int = _abi.PATH_AUTO, flags: int = 0, max_bounces: int = 0):
    cell = min(vol.GetCellSize() for vol in sc.volumes())
    p = v.default_params(WIDTH, HEIGHT, cell, v.march_budget(RESOLUTION, 255), shadow=True, mode=mode, path=path)
    p.flags = flags
    p.max_bounces = max_bounces
    return p


def all_pixels() -> np.ndarray:
    return np.array([(x, y) for y in range(HEIGHT) for x in range(WIDTH)], np.int32)
