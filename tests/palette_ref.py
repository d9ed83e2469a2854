"""Plain-numpy restatement of the rule by which a hit on a slot with a palette gets its entry (include/vrt.h, vrt_volume_set_palette),
written from the header rather than from the kernel, and the painted sphere the palette tests render.

entry_ids() takes a downloaded volume (decoded densities and material ids, both [x, z, y]) and object-space hit points and returns, per
point, the material id the rule picks and the point's distance, in cells, to the nearest place where the rule's decision changes: a cell
face (the cell c changes), the bisector plane of the best INSIDE corner and any other INSIDE corner (the chosen corner changes — the two
best corners' bisector among them) or, in a cell without an INSIDE corner, a half-cell plane of the nearest-sample rule.  The device
computes the hit point in fp32 with its own rounding; a test compares only where that distance exceeds a margin far above fp32 rounding.
Every operation on g, c and f is an np.float32 operation in the header's parenthesisation.

Further down: the seven-point criterion that names the compared pixels of a Cube mode without knowing the rule, the header's Cube-mode
step (hit_cells), the scenes of tests/test_volume_palette_paths_gpu.py, which their twins in tests/test_volume_palette.py put under the
CPU oracle, and the helpers the two GPU suites share (frames, U_k, check_composition)."""
from __future__ import annotations

import math

import numpy as np

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

import volume_ref

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


CUBE_SNAP = f32(2.0 ** -8)   # cells: how near to an integer g is along the axis of the face a Cube-mode hit lies on (vrt.h)


def object_directions(rotation, scale, directions) -> np.ndarray:
    """The object-space ray directions w2o d (float64), as object_points uses them."""
    d = np.asarray(directions, np.float64).reshape(-1, 3) / np.asarray(scale, np.float64)
    qi = v.quat_inverse(rotation)
    return np.stack([v.quat_rotate(qi, x) for x in d]).astype(np.float64)


def hit_cells(N: int, extent: float, points_xyz, cube_directions=None):
    """Step 1 of the rule: (g [n, 3] fp32, c [n, 3] int, face distance [n] float64: how far, in cells, g is from where c would change).
    cube_directions: the object-space ray directions of Cube-mode hits — along the axis on which g is nearest to an integer k (the
    lowest on a tie), if within 2^-8 of it, the cell is k's on the side the ray travels to: k - 1 for a negative direction, else k."""
    cell = f32(f32(extent) * f32(2.0)) / f32(N - 1)
    inv_cell = f32(1.0) / cell
    p = np.asarray(points_xyz, np.float64).reshape(-1, 3).astype(f32)
    g = ((p + f32(extent)) * inv_cell).astype(f32)                       # g_a = (p_a + extent) * inv_cell
    q = np.floor(g)
    G = g.astype(np.float64)
    face = np.minimum(G - np.floor(G), 1.0 - (G - np.floor(G)))          # per axis, to the planes where floor(g_a) changes
    if cube_directions is not None:
        od = np.asarray(cube_directions, np.float64).reshape(-1, 3).astype(f32)
        k = np.rint(g).astype(f32)
        a = np.abs(g - k).astype(f32)
        axis = np.argmin(a, axis=1)                                      # the first (lowest) of equal minima
        rows = np.arange(len(g))
        snap = a[rows, axis] <= CUBE_SNAP
        side = np.where(od[rows, axis] < 0, k[rows, axis] - f32(1.0), k[rows, axis])
        q[rows[snap], axis[snap]] = side[snap]
        # on the snapped axis the choice changes only where |g - k| reaches 2^-8, or where another axis comes as near to an integer
        # (that axis' own face distance); without a snap, where the nearest axis comes within 2^-8
        near = np.abs(a[rows, axis].astype(np.float64) - float(CUBE_SNAP))
        face[rows[snap], axis[snap]] = near[snap]
        face[rows[~snap], axis[~snap]] = np.minimum(face[rows[~snap], axis[~snap]], near[~snap])
    c = np.clip(q, f32(0), f32(N - 2)).astype(np.int64)                  # c_a = clamp(floor(g_a), 0, N-2)
    return g, c, face.min(axis=1)


def entry_ids(density: np.ndarray, material: np.ndarray, extent: float, points_xyz, cube_directions=None):
    """(ids [n] int, boundary distance in cells [n] float64) of the object-space points; density: the DECODED densities [x, z, y] (a
    VRT_FORMAT_TEXEL16 slot's q * 0.01f keeps the stored field's sign, -0.0 included), material: uint8 [x, z, y].  cube_directions: the
    points are Cube-mode hits of rays with these object-space directions (hit_cells)."""
    N = density.shape[0]
    g, c, face = hit_cells(N, extent, points_xyz, cube_directions)
    n = len(g)
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
    dist = np.minimum(F, 1.0 - F).min(axis=1) if cube_directions is None else face   # cell faces
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


# ---- a second criterion for the Cube modes -----------------------------------------------------------------------------------------
CUBE_EXCLUDED_CAP = 0.05   # the share of hit pixels the seven-point criterion may leave out in a Cube mode
ID_SHARE = 0.10            # every id a test requires shows on at least this share of its instance's hit pixels


def seven_point_ids(density: np.ndarray, material: np.ndarray, extent: float, points_xyz):
    """(ids [n] int, same [n] bool): entry_ids' id of every object-space point p, and whether entry_ids names that id at all seven of
    p, p +- m e_x, p +- m e_y, p +- m e_z, m = MARGIN_CELLS cells.  It asks nothing of the rule but its answers: a Cube-mode hit lies on
    a cell face, where step 1's floor is decided by how the hit point was rounded, and is compared where the cells on both sides of
    that face (and of any other face, bisector or half-cell plane within m) give the same id."""
    N = density.shape[0]
    m = MARGIN_CELLS * (2.0 * float(extent) / (N - 1))
    p = np.asarray(points_xyz, np.float64).reshape(-1, 3)
    ids, _ = entry_ids(density, material, extent, p)
    same = np.ones(len(p), bool)
    for a in range(3):
        for s in (-m, m):
            q = p.copy()
            q[:, a] += s
            same &= entry_ids(density, material, extent, q)[0] == ids
    return ids, same


def seven_point_dist(density, material, extent, points_xyz):
    """seven_point_ids in the shape of entry_ids: a 'distance' of +inf where the seven ids agree and 0 where they do not."""
    ids, same = seven_point_ids(density, material, extent, points_xyz)
    return ids, np.where(same, np.inf, 0.0)


# ---- the scenes of tests/test_volume_palette_paths_gpu.py, shared with their twins under the oracle ---------------------------------------
T16 = _abi.FORMAT_TEXEL16
BESIDE_AT = (-22.0, -4.0, -1.0)   # where the second, palette-free object stands


def decoded_density(vol: v.VVoxelVolume) -> np.ndarray:
    """The densities the device decodes for vol as uploaded: its own, or (VRT_FORMAT_TEXEL16) the integer field +-q times 0.01f."""
    if vol.device_format != T16:
        return np.asarray(vol.density, f32)
    return (volume_ref.texel16_field(vol.density) * f32(0.01)).astype(f32)


def paint_on_host(vol: v.VVoxelVolume, axis: int = 0, plane: float = PAINT_X) -> v.VVoxelVolume:
    """What the PAINT box leaves (test_the_test_scenes_exclusion_share_and_both_ids pins the box to this): id 1 on the INSIDE samples
    (decoded density <= 0), id 2 on those beyond `plane` along grid axis `axis` (0: x, 1: y, 2: z), id 0 outside."""
    inside = decoded_density(vol) <= 0
    shape = [1, 1, 1]
    shape[(0, 2, 1)[axis]] = vol.N        # arrays are [x, z, y]
    beyond = (np.arange(vol.N) > plane).reshape(shape)
    vol.material_id = np.where(inside, np.where(beyond, 2, 1), 0).astype(np.uint8)
    vol.dirty = True
    return vol


def plain_sphere(radius_cells: float = 7.5, fmt: int = _abi.FORMAT_F32, material=((0.5, 0.7, 0.3, 1.0), 0.7, 0.1)) -> v.VVoxelVolume:
    """A smaller rough sphere without a palette: the second object of the mixed-format and mirror scenes, slot 0 of the slots scene."""
    vol = v.VVoxelVolume(RESOLUTION, EXTENT)
    vol.fill(lambda X, Y, Z: np.sqrt((X * X + Y * Y) + Z * Z).astype(f32) - f32(radius_cells))
    vol.set_device_format(fmt)
    vol.Material = v.VMaterial(tuple(material[0]), material[1], material[2])
    return vol


class SlotScene(v.VScene):
    """A scene whose volume slots are given (slot_volumes) rather than taken in first-use order, so that instance i need not use slot i."""
    slot_volumes = ()

    def volumes(self):
        return list(self.slot_volumes)


# item 1: name -> (format of the painted sphere, path, mode, format of a second object or None); the kernel path follows resolve_path
CASES = {
    "brick": (_abi.FORMAT_F32, _abi.PATH_BRICK, _abi.MODE_INTERP_NOTEX, None),     # VRT_PATH_BRICK
    "dense": (_abi.FORMAT_F32, _abi.PATH_DENSE, _abi.MODE_INTERP_NOTEX, None),     # VRT_PATH_DENSE
    "brick16": (T16, _abi.PATH_BRICK, _abi.MODE_INTERP_NOTEX, None),               # every slot TEXEL16: kPathBrick16
    "cells16": (T16, _abi.PATH_CELLS, _abi.MODE_INTERP_NOTEX, None),               # every slot TEXEL16: kPathCells16
    "mixed": (T16, _abi.PATH_BRICK, _abi.MODE_INTERP_NOTEX, _abi.FORMAT_F32),      # mixed formats: VRT_PATH_DENSE over a +-q field
    "cube": (_abi.FORMAT_F32, _abi.PATH_AUTO, _abi.MODE_CUBE_NOTEX, None),         # a Cube mode: kPathCube
    "cube16": (T16, _abi.PATH_AUTO, _abi.MODE_CUBE_NOTEX, None),                   # a Cube mode, every slot TEXEL16: kPathCube16
}


def is_cube(p) -> bool:
    return p.mode >= _abi.MODE_CUBE


def ids_of(vol_density, vol_material, p, points):
    """(ids, boundary distance) by the criterion of the mode: entry_ids' own distance, or the seven points in a Cube mode."""
    return (seven_point_dist if is_cube(p) else entry_ids)(vol_density, vol_material, EXTENT, points)


def excluded_cap(p) -> float:
    return CUBE_EXCLUDED_CAP if is_cube(p) else EXCLUDED_CAP


def camera_along(target, direction, distance: float, fov: float) -> v.VCamera:
    """A camera `distance` from `target`, looking at it along `direction` (world space)."""
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    q = v.quat_mul(v.quat_from_axis_angle(v.UP, math.atan2(d[1], d[0])), v.quat_from_axis_angle(v.RIGHT, -math.asin(d[2])))
    assert np.allclose(v.quat_rotate(q, v.FORWARD), d, atol=1e-6)
    return v.VCamera(Position=tuple(float(x) for x in np.asarray(target, np.float64) - distance * d), Rotation=tuple(q), FOVAngle=fov)


# The Cube cases look at the sphere along CUBE_VIEW, given in the sphere's OBJECT space: every camera ray then runs towards +x, +y and +z
# there and enters a solid cell through one of its low faces, whose corners the cell before it shares — the seven-point criterion keeps
# such a hit wherever the nearest INSIDE sample is one of them.  (Through a high face the cell before has other corners, mostly none of
# them INSIDE: test_a_cube_hit_renders_the_entered_cell covers those with the rule itself.)
CUBE_VIEW, CUBE_DISTANCE, CUBE_FOV = (0.3, 0.62, 0.72), 70.0, 24.0


def case_scene(name: str, flags: int = 0, max_bounces: int = 0, cube_view=CUBE_VIEW):
    """(scene, params, the painted volume) of an item-1 case: the painted sphere (slot 0, instance 0), painted on the host."""
    fmt, path, mode, second = CASES[name]
    vol = paint_on_host(sphere_volume(fmt))
    vol.Material = v.VMaterial(tuple(ENTRIES[0][0]), ENTRIES[0][1], ENTRIES[0][2])
    sc = painted_sphere_scene(vol)
    if mode >= _abi.MODE_CUBE and cube_view is not None:
        obj = sc.Objects[0]
        world = np.asarray(v.quat_rotate(obj.Rotation, np.asarray(cube_view, np.float64) * np.asarray(obj.Scale, np.float64)), np.float64)
        sc.Camera = camera_along(obj.Position, world, CUBE_DISTANCE, CUBE_FOV)
    if second is not None:
        sc.Objects.append(v.VVoxelObject(Position=BESIDE_AT, Rotation=tuple(v.quat_from_axis_angle(v.UP, 0.6)), Volume=plain_sphere(fmt=second)))
    return sc, scene_params(sc, mode=mode, path=path, flags=flags, max_bounces=max_bounces), vol


def moved(sc: v.VScene) -> v.VScene:
    """The scene with its first object moved: frame 1 of a block with per-frame scenes."""
    objs = [v.VVoxelObject(Position=o.Position, Rotation=o.Rotation, Scale=o.Scale, Volume=o.Volume) for o in sc.Objects]
    objs[0].Position = (objs[0].Position[0] + 2.0, objs[0].Position[1], objs[0].Position[2])
    out = type(sc)(Camera=sc.Camera, DirectionalLight=sc.DirectionalLight, Objects=objs, PointLights=sc.PointLights,
                   SpotLights=sc.SpotLights, EnvironmentMap=sc.EnvironmentMap)
    if isinstance(sc, SlotScene):
        out.slot_volumes = sc.slot_volumes
    return out


# item 3: three slots, four instances [slot 2, slot 0, slot 1, slot 1], two palettes of different lengths
PALETTE_A = ENTRIES
PALETTE_B = (((0.9, 0.8, 0.1, 1.0), 0.6, 0.3), ((0.2, 0.8, 0.7, 1.0), 0.45, 0.2))
SLOT2_OWN = ((0.6, 0.2, 0.7, 1.0), 0.55, 0.4)   # what slot 2's id 2, beyond palette B, renders
PAINT_Z = 15.6
SLOTS_INSTANCES = (2, 0, 1, 1)


def slots_scene():
    """(scene, params, [slot 0, slot 1, slot 2]): the four spheres stand side by side (a 2 x 2 grid under a camera on +Y), apart by more
    than their diameters; all materials rough."""
    plain = plain_sphere(9.0)
    a = paint_on_host(sphere_volume())
    a.Material = v.VMaterial(tuple(PALETTE_A[0][0]), PALETTE_A[0][1], PALETTE_A[0][2])
    b = paint_on_host(sphere_volume(), axis=2, plane=PAINT_Z)
    b.Material = v.VMaterial(tuple(SLOT2_OWN[0]), SLOT2_OWN[1], SLOT2_OWN[2])
    vols = [plain, a, b]
    at = ((-13.0, 0.0, 12.5), (13.0, 0.5, 12.0), (-13.5, -0.5, -12.0), (13.0, 0.0, -12.5))
    yaw = (0.35, 0.0, -0.5, 0.9)
    scale = ((1.05, 1.0, 0.95), (1.0, 1.0, 1.0), (1.1, 1.0, 0.9), (0.9, 1.05, 1.0))
    objs = [v.VVoxelObject(Position=at[i], Rotation=tuple(v.quat_from_axis_angle(v.UP, yaw[i])), Scale=scale[i], Volume=vols[s])
            for i, s in enumerate(SLOTS_INSTANCES)]
    base = painted_sphere_scene(a)
    cam = v.VCamera(Position=(0.0, 58.0, 5.0), Rotation=base.Camera.Rotation, FOVAngle=60.0)
    sc = SlotScene(Camera=cam, DirectionalLight=base.DirectionalLight, Objects=objs, SpotLights=base.SpotLights, EnvironmentMap=base.EnvironmentMap)
    sc.slot_volumes = tuple(vols)
    return sc, scene_params(sc), vols


def instance_of_points(sc: v.VScene, origins, directions, t) -> np.ndarray:
    """The instance each hit lies on, from the geometry alone (the oracle's batch trace does not name it): the one in whose object space
    the hit point is nearest to the origin, the objects being apart."""
    r = np.stack([np.linalg.norm(object_points(o.Position, o.Rotation, o.Scale, origins, directions, t), axis=1) for o in sc.Objects])
    return np.argmin(r, axis=0)


# item 4: the mirror decision per pixel
MIRROR_ENTRY = (ENTRIES[1][0], 0.1, 0.9)
ONLY_AN_ENTRY_MIRRORS = (ENTRIES[0], MIRROR_ENTRY, ENTRIES[2])              # (a) the slot's material: ENTRIES[0], rough
ONLY_THE_SLOT_MIRRORS = (ENTRIES[0], ENTRIES[1])                            # (b) the slot's material: SLOT_MIRROR, id 2 beyond the palette
SLOT_MIRROR = ((0.3, 0.8, 0.4, 1.0), 0.1, 0.7)


def bounce_scene():
    """(scene, params, the painted volume): the painted sphere beside a rough sphere without a palette, two bounces allowed.  The sphere
    is scaled uniformly here: stretched (1.1, 1.0, 0.9) its normals lean enough for 7 of 732 reflected rays to meet it again, and the
    bounce count of a frame is the number of mirroring pixels only while no reflected ray returns (the twin under the oracle holds the
    scene to that)."""
    vol = paint_on_host(sphere_volume())
    vol.Material = v.VMaterial(tuple(ENTRIES[0][0]), ENTRIES[0][1], ENTRIES[0][2])
    sc = painted_sphere_scene(vol)
    sc.Objects[0].Scale = (1.05, 1.05, 1.05)
    sc.Objects.append(v.VVoxelObject(Position=BESIDE_AT, Rotation=tuple(v.quat_from_axis_angle(v.UP, 0.6)), Volume=plain_sphere()))
    return sc, scene_params(sc, flags=_abi.FLAG_FULL_ONE_KERNEL, max_bounces=2), vol


# item 5: the raw pair.  2 x 2 textures; the rm texture's R scales the roughness by 2/3 or 1 (0.35 crosses 0.3, 0.5 and 0.8 do not), its G
# the metallic
ALBEDO_TEX = np.array([[[255, 255, 255, 255], [60, 200, 90, 255]], [[200, 80, 220, 255], [30, 30, 160, 255]]], np.uint8)
NORMAL_TEX = np.array([[[128, 128, 255, 255], [150, 120, 240, 255]], [[110, 140, 245, 255], [128, 100, 235, 255]]], np.uint8)
RM_TEX = np.array([[[170, 255, 0, 255], [255, 128, 0, 255]], [[255, 255, 0, 255], [170, 64, 0, 255]]], np.uint8)


def textured_scene():
    vol = paint_on_host(sphere_volume())
    vol.Material = v.VMaterial(tuple(ENTRIES[0][0]), ENTRIES[0][1], ENTRIES[0][2], AlbedoTexture=ALBEDO_TEX, NormalTexture=NORMAL_TEX,
                               RMTexture=RM_TEX, TextureScale=(7.0, 5.0))
    sc = painted_sphere_scene(vol)
    return sc, scene_params(sc, mode=_abi.MODE_INTERP, flags=_abi.FLAG_FULL_ONE_KERNEL, max_bounces=1), vol


# step 3's other branch: a cell without an INSIDE corner.  From far away the cone threshold stops a ray well short of the surface, often in
# the cell outside it; the OUTSIDE samples carry ids here (0 and 1 by the parity of x + y + z, so that neighbours differ), which no
# edit call writes but an upload may
FAR_DISTANCE, FAR_FOV, FAR_VIEW = 140.0, 15.0, (0.05, -1.0, -0.17)


def far_scene(flags: int = 0):
    vol = paint_on_host(sphere_volume())
    i = np.arange(vol.N)
    odd = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) & 1).astype(np.uint8)
    vol.material_id = np.where(vol.material_id == 0, odd, vol.material_id).astype(np.uint8)
    vol.Material = v.VMaterial(tuple(ENTRIES[0][0]), ENTRIES[0][1], ENTRIES[0][2])
    sc = painted_sphere_scene(vol)
    sc.Camera = camera_along(sc.Objects[0].Position, FAR_VIEW, FAR_DISTANCE, FAR_FOV)
    return sc, scene_params(sc, flags=flags), vol


def without_inside_corner(density, material, extent, points_xyz):
    """(mask [n]: the point's cell has no INSIDE corner, so that step 3 names the nearest sample; the id of that cell's corner 0 [n])."""
    _, c, _ = hit_cells(density.shape[0], extent, points_xyz)
    inside = np.zeros(len(c), bool)
    with np.errstate(invalid="ignore"):
        for j in range(8):
            inside |= density[c[:, 0] + (j & 1), c[:, 2] + (j >> 2), c[:, 1] + ((j >> 1) & 1)] <= f32(0)
    return ~inside, material[c[:, 0], c[:, 2], c[:, 1]].astype(np.int64)


# item 7: zeros of both signs and the last id
ZERO_BAND = 0.15                       # samples with |density| below this many cells become -0 / +0
ZERO_IDS = (1, 254, 2, 255)            # id of an INSIDE sample: ZERO_IDS[(x + y + z) % 4], so neighbours along an axis differ


def zeros_volume(fmt: int) -> v.VVoxelVolume:
    """The sphere with the samples of a thin band about its surface set to -0 and +0 alternately (F32: the zeros themselves; TEXEL16:
    -0.004 and +0.004, which the quantiser stores as -0 and +0), ids from density <= 0 — both zeros are INSIDE."""
    vol = sphere_volume(fmt)
    d = np.array(vol.density, f32)
    i = np.arange(vol.N)
    parity = (i[:, None, None] + i[None, :, None] + i[None, None, :])
    band = np.abs(d) < f32(ZERO_BAND)
    z = f32(0.004) if fmt == T16 else f32(0.0)
    d[band] = np.where(parity[band] & 1, -z, z)
    vol.density = d
    inside = decoded_density(vol) <= 0
    vol.material_id = np.where(inside, np.array(ZERO_IDS, np.uint8)[parity % 4], 0).astype(np.uint8)
    vol.dirty = True
    return vol


def zeros_palette():
    """256 entries, all rough, each of the ZERO_IDS and entry 0 with a colour of its own, 255 the most distinct."""
    e = [((0.2 + 0.6 * (k % 7) / 6.0, 0.3 + 0.5 * (k % 5) / 4.0, 0.25 + 0.5 * (k % 3) / 2.0, 1.0), 0.4 + 0.5 * (k % 11) / 10.0, 0.1 * (k % 4)) for k in range(256)]
    e[255] = ((1.0, 0.05, 0.6, 1.0), 0.33, 0.9)
    e[254] = ((0.05, 0.9, 0.2, 1.0), 0.7, 0.0)
    return e


def zeros_scene(fmt: int):
    vol = zeros_volume(fmt)
    vol.Material = v.VMaterial((0.5, 0.5, 0.5, 1.0), 0.6, 0.0)
    sc = painted_sphere_scene(vol)
    return sc, scene_params(sc, flags=_abi.FLAG_FULL_ONE_KERNEL), vol


# ---- what the GPU suites share: a renderer in, frames and comparisons out -----------------------------------------------------------------
PARITY_TOL = 1e-4   # the parity tolerance of tests/test_parity_gpu.py


def use(r, sc, p):
    """The scene synced, and no palette left on its slots by an earlier test (a palette stays with its slot like the material)."""
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)
    r.SyncWithScene()
    for slot in range(len(sc.volumes())):
        r.set_palette(slot, None)


def frame(r):
    img = r.Render().copy()
    return img, r.last_timing(), r.last_kernel_form()


def bits(img):
    return np.ascontiguousarray(img, np.float32).view(np.uint32)


def material_of(entry, like: v.VMaterial = None) -> v.VMaterial:
    """The entry as a slot's material, with the textures of `like`."""
    m = v.VMaterial(tuple(entry[0]), entry[1], entry[2])
    if like is not None:
        m.AlbedoTexture, m.NormalTexture, m.RMTexture, m.TextureScale = like.AlbedoTexture, like.NormalTexture, like.RMTexture, like.TextureScale
    return m


def camera_hits(r, p):
    rays = r.camera_rays(all_pixels(), p.width, p.height)
    got = r.trace_rays(rays["origin"], rays["direction"], params=p)
    return rays, got


def uniform_frames(r, vol, entries, also=(), oracle=None, timings=None):
    """U_k: no palette, the slot's material = entry k, the full closest hit in one kernel.  also: (volume, entries) of further slots, set
    along with it; oracle: (scene, params) — every U_k is then held to the CPU oracle's frame of the same scene within PARITY_TOL;
    timings: a list that receives each frame's counters."""
    from oracle.binding import OracleScene

    out = []
    slots = [(vol, entries)] + list(also)
    keep = [x.Material for x, _ in slots]
    for k in range(len(entries)):
        for (x, e), own in zip(slots, keep):
            x.Material = material_of(e[k], own)
        img, t, form = frame(r)
        assert form & _abi.FORM_FULL and not form & (_abi.FORM_PALETTE | _abi.FORM_PASSES)
        if oracle is not None:
            ref, _ = OracleScene(oracle[0]).render(oracle[1], threads=8)
            err = float(np.abs(img - ref).max())
            print(f"U_{k} against the oracle: max |difference| {err:.3e}")
            assert err <= PARITY_TOL
        if timings is not None:
            timings.append(t)
        out.append(img)
    for (x, _), own in zip(slots, keep):
        x.Material = own
    return out


def check_composition(P, U, ids, dist, hit_idx, n_hit, need=(1, 2), cap=EXCLUDED_CAP, what=""):
    """P == U[id] bit for bit at every hit pixel (flat indices hit_idx) whose boundary distance exceeds the margin; the pixels left out
    stay below `cap` of the n_hit hit pixels and every id of `need` is compared on at least ID_SHARE of them.  Returns the mask of the
    compared ones."""
    ok = dist >= MARGIN_CELLS
    excluded = int((~ok).sum())
    Pb = bits(P).reshape(-1, 4)
    wrong = 0
    for k in sorted(set(ids[ok].tolist())):
        sel = hit_idx[ok & (ids == k)]
        wrong += int(np.any(Pb[sel] != bits(U[k]).reshape(-1, 4)[sel], axis=1).sum())
    counts = {k: int((ids == k).sum()) for k in sorted(set(ids.tolist()))}
    print(f"{what}hit pixels {n_hit}, compared {int(ok.sum())}, excluded {excluded} ({100.0 * excluded / max(n_hit, 1):.2f} %), wrong {wrong}, ids {counts}")
    assert excluded < cap * n_hit
    for k in need:
        assert int((ok & (ids == k)).sum()) >= ID_SHARE * n_hit, k
    assert wrong == 0
    return ok
