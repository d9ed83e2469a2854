"""Python host wrapper over the C-ABI: the `VRenderer` surface of the reference
(Renderer/Public/Renderer.h:44-66 — Start/Stop/IsActive/SetSceneToRender/Render/
ResizeRenderOutput/SetRendererMode) for the HIP backend.  Used by tests and bench.py; the C++
adaptor with the same shape is csrc/host/HipRenderer.h.

Everything here calls into libvrt_hip.so.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _abi
from .scene import VScene, VVoxelVolume, default_params, march_budget


# numpy views of vrt_ray / vrt_hit (include/vrt.h)
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("reserved_", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("instance", "<i4"), ("voxel", "<i4", 3), ("material", "<u4"),
                      ("steps", "<u4"), ("reserved_", "<u4", 2)])
assert RAY_DTYPE.itemsize == C.sizeof(_abi.vrt_ray) and HIT_DTYPE.itemsize == C.sizeof(_abi.vrt_hit)
POINT_DTYPE = np.dtype([("position", "<f4", 3), ("reserved_", "<f4")])
POINT_RESULT_DTYPE = np.dtype([("distance", "<f4"), ("normal", "<f4", 3), ("instance", "<i4"), ("voxel", "<i4", 3), ("material", "<u4"),
                               ("flags", "<u4"), ("moves", "<u4"), ("position", "<f4", 3), ("reserved_", "<u4", 2)])
assert POINT_DTYPE.itemsize == C.sizeof(_abi.vrt_point) and POINT_RESULT_DTYPE.itemsize == C.sizeof(_abi.vrt_point_result)
CONTACT_DTYPE = np.dtype([("position", "<f4", 3), ("distance", "<f4"), ("normal", "<f4", 3), ("material_a", "<u4"), ("normal_a", "<f4", 3),
                          ("material_b", "<u4"), ("cell_a", "<i4", 3), ("reserved_", "<u4")])
assert CONTACT_DTYPE.itemsize == C.sizeof(_abi.vrt_contact)


def make_points(points) -> np.ndarray:
    """A vrt_point array from [n, 3] world-space positions."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(p), POINT_DTYPE)
    out["position"] = p
    return out


def point_results_to_dict(res: np.ndarray) -> dict:
    """The fields of a vrt_point_result array as separate numpy arrays; sampled = flags & VRT_POINT_SAMPLED."""
    return {"distance": res["distance"].copy(), "normal": res["normal"].copy(), "instance": res["instance"].copy(),
            "voxel": res["voxel"].copy(), "material": res["material"].copy(), "sampled": (res["flags"] & _abi.POINT_SAMPLED) != 0,
            "moves": res["moves"].copy(), "position": res["position"].copy()}


SWEEP_DTYPE = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("radius", "<f4")])
SWEEP_HIT_DTYPE = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("instance", "<i4"), ("voxel", "<i4", 3), ("material", "<u4"), ("flags", "<u4"),
                            ("steps", "<u4"), ("distance", "<f4"), ("position", "<f4", 3), ("reserved_", "<u4")])
assert SWEEP_DTYPE.itemsize == C.sizeof(_abi.vrt_sweep) and SWEEP_HIT_DTYPE.itemsize == C.sizeof(_abi.vrt_sweep_hit)


def make_sweeps(origins, directions, radius=0.0, t_max=10000.0) -> np.ndarray:
    """A vrt_sweep array from [n, 3] origins and directions and a scalar or per-record radius and t_max."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("origins and directions differ in length")
    out = np.zeros(len(o), SWEEP_DTYPE)
    out["origin"], out["direction"] = o, d
    out["radius"] = np.broadcast_to(np.asarray(radius, dtype=np.float32), (len(o),))
    out["t_max"] = np.broadcast_to(np.asarray(t_max, dtype=np.float32), (len(o),))
    return out


def sweep_hits_to_dict(res: np.ndarray) -> dict:
    """The fields of a vrt_sweep_hit array as separate numpy arrays; hit, exhausted and initial are the bits of flags."""
    out = {k: res[k].copy() for k in ("t", "normal", "instance", "voxel", "material", "flags", "steps", "distance", "position")}
    out["hit"] = (res["flags"] & _abi.SWEEP_HIT) != 0
    out["exhausted"] = (res["flags"] & _abi.SWEEP_EXHAUSTED) != 0
    out["initial"] = (res["flags"] & _abi.SWEEP_INITIAL) != 0
    return out


def contacts_to_dict(rec: np.ndarray, res: "_abi.vrt_contacts_result") -> dict:
    """A CONTACT_DTYPE array and its vrt_contacts_result as one dict: the records' fields as separate numpy arrays, and the result's."""
    out = {k: rec[k].copy() for k in ("position", "distance", "normal", "material_a", "normal_a", "material_b", "cell_a")}
    out.update(_abi.contacts_result_dict(res))
    return out


def make_rays(origins, directions, t_max=10000.0) -> np.ndarray:
    """A vrt_ray array from [n, 3] origins and directions and a scalar or per-ray t_max."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("origins and directions differ in length")
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["t_max"] = np.broadcast_to(np.asarray(t_max, dtype=np.float32), (len(o),))
    return rays


def hits_to_dict(hits: np.ndarray) -> dict:
    """The fields of a vrt_hit array as separate numpy arrays; hit = instance >= 0."""
    return {"hit": hits["instance"] >= 0, "t": hits["t"].copy(), "normal": hits["normal"].copy(), "instance": hits["instance"].copy(),
            "voxel": hits["voxel"].copy(), "material": hits["material"].copy(), "steps": hits["steps"].copy()}


def _brush(shape, op, a, b, radius, blend, reach, material) -> _abi.vrt_brush:
    r = _abi.vrt_brush()
    r.shape, r.op = int(shape), int(op)
    for i in range(3):
        r.a[i], r.b[i] = float(a[i]), float(b[i])
    r.radius, r.blend, r.reach, r.material = float(radius), float(blend), float(reach), int(material)
    return r


def sphere_brush(op: int, center, radius: float, blend: float = 0.0, reach: float = 2.0, material: int = -1) -> _abi.vrt_brush:
    """A vrt_brush record: a sphere at `center` (grid coordinates xyz, fractions allowed), lengths in cells (vrt.h)."""
    return _brush(_abi.BRUSH_SPHERE, op, center, (0.0, 0.0, 0.0), radius, blend, reach, material)


def box_brush(op: int, center, half_sizes, rounding: float = 0.0, blend: float = 0.0, reach: float = 2.0,
              material: int = -1) -> _abi.vrt_brush:
    """A vrt_brush record: an axis-aligned box of `half_sizes` (xyz, cells) at `center`, its corners rounded by `rounding`."""
    return _brush(_abi.BRUSH_BOX, op, center, half_sizes, rounding, blend, reach, material)


def capsule_brush(op: int, end_a, end_b, radius: float, blend: float = 0.0, reach: float = 2.0, material: int = -1) -> _abi.vrt_brush:
    """A vrt_brush record: the capsule of `radius` around the segment end_a..end_b (grid coordinates xyz)."""
    return _brush(_abi.BRUSH_CAPSULE, op, end_a, end_b, radius, blend, reach, material)


def smooth_record(shape: int, a, b, radius: float, strength: float = 0.5, iterations: int = 1, falloff: float = 1.0, rebound: float = 0.0,
                  material: int = -1) -> _abi.vrt_smooth:
    """A vrt_smooth record: the region is the shape of a brush record (BRUSH_SPHERE: centre a, b ignored; BRUSH_BOX: centre a, half
    sizes b, rounding `radius`; BRUSH_CAPSULE: ends a and b), lengths in cells, positions in grid coordinates xyz (vrt.h)."""
    r = _abi.vrt_smooth()
    r.shape, r.iterations, r.material = int(shape), int(iterations), int(material)
    for i in range(3):
        r.a[i], r.b[i] = float(a[i]), float(b[i])
    r.radius, r.strength, r.falloff, r.rebound = float(radius), float(strength), float(falloff), float(rebound)
    return r


def _inverse_turn_and_scale(rotation_xyzw, scale: float, who: str) -> np.ndarray:
    """R^T / scale in double, R being the turn of the quaternion (any length but 0)."""
    x, y, z, w = (float(c) for c in rotation_xyzw)
    n = (x * x + y * y + z * z + w * w) ** 0.5
    if not n > 0.0 or not float(scale) > 0.0:
        raise ValueError(f"{who}: a zero quaternion or a scale that is not positive")
    x, y, z, w = x / n, y / n, z / n, w / n
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)
    return rot.T / float(scale)


IDENTITY_PULL = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def warp_record(shape: int, a, b, radius: float, pull=IDENTITY_PULL, length_scale: float = 1.0, inflate: float = 0.0, strength: float = 1.0,
                falloff: float = 1.0, material: int = _abi.WARP_MATERIAL_KEEP) -> _abi.vrt_warp:
    """A vrt_warp record: the region is the shape of a brush record (as smooth_record takes it); pull is the row-major 3x4 matrix (12
    values, or a [3, 4] array) that says where a sample at full weight takes its value FROM, in grid coordinates xyz — the inverse of
    the motion one sees (warp_from_motion builds it); inflate in cells (vrt.h)."""
    m = np.asarray(pull, dtype=np.float64).reshape(12)
    r = _abi.vrt_warp()
    r.shape, r.material = int(shape), int(material)
    for i in range(3):
        r.a[i], r.b[i] = float(a[i]), float(b[i])
    for i in range(12):
        r.pull[i] = float(m[i])
    r.radius, r.strength, r.falloff, r.length_scale, r.inflate = float(radius), float(strength), float(falloff), float(length_scale), float(inflate)
    return r


def warp_from_motion(pivot, translation=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0, 1.0), scale: float = 1.0):
    """(pull, length_scale) of a vrt_warp record for the motion one sees: a turn by the quaternion `rotation` (xyzw) and a uniform
    `scale` about `pivot` (grid coordinates xyz), then a shift by `translation` (cells) — p' = pivot + scale R (p - pivot) +
    translation.  pull is the inverse motion, p = pivot + R^T (p' - pivot - translation) / scale, built in double; pull is a [3, 4]
    float64 array that warp_record rounds to fp32 once; length_scale = scale."""
    lin = _inverse_turn_and_scale(rotation, scale, "warp_from_motion")
    c = np.asarray(pivot, np.float64).reshape(3)
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = lin
    m[:, 3] = c - lin @ (c + np.asarray(translation, np.float64).reshape(3))
    return m, float(scale)


def stamp_record(op: int, dst_to_src, length_scale: float = 1.0, offset: float = 0.0, blend: float = 0.0, reach: float = 2.0,
                 material: int = _abi.STAMP_MATERIAL_KEEP) -> _abi.vrt_stamp:
    """A vrt_stamp record from the matrix itself: dst_to_src is the row-major 3x4 matrix (12 values, or a [3, 4] array) that takes
    destination grid coordinates (x, y, z) to source grid coordinates; lengths in cells of the destination (vrt.h)."""
    m = np.asarray(dst_to_src, dtype=np.float64).reshape(12)
    r = _abi.vrt_stamp()
    r.op, r.material = int(op), int(material)
    for i in range(12):
        r.dst_to_src[i] = float(m[i])
    r.length_scale, r.offset, r.blend, r.reach = float(length_scale), float(offset), float(blend), float(reach)
    return r


def stamp_from_placement(src_N: int, position, rotation_xyzw=(0.0, 0.0, 0.0, 1.0), scale: float = 1.0, op: int = _abi.STAMP_ADD,
                         offset: float = 0.0, blend: float = 0.0, reach: float = 2.0, material: int = _abi.STAMP_MATERIAL_KEEP) -> _abi.vrt_stamp:
    """A vrt_stamp record that places a source of src_N^3 samples in the destination's grid: the source's centre sample sits at
    `position` (destination grid coordinates xyz, fractions allowed), turned by the quaternion `rotation_xyzw` about it, and one
    source cell covers `scale` destination cells.  The matrix u = R^T (p - position) / scale + (src_N - 1) / 2 is built in double
    and rounded to fp32 once; length_scale = scale."""
    lin = _inverse_turn_and_scale(rotation_xyzw, scale, "stamp_from_placement")
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = lin
    m[:, 3] = -lin @ np.asarray(position, np.float64).reshape(3) + (int(src_N) - 1) / 2.0
    return stamp_record(op, m, scale, offset, blend, reach, material)


class VHipRenderer:
    def __init__(self, devices: Sequence[int] = (0,)):
        self._lib = _abi.load()
        self._devices = list(devices)
        self._ctx = C.c_void_p()
        self._scene: Optional[VScene] = None
        self._slots: List[VVoxelVolume] = []
        self._uploaded: Dict[int, int] = {}  # slot -> id(volume) currently on the device
        self.RenderMode = _abi.MODE_INTERP
        self.Width, self.Height = 1024, 576  # default window, UI/Win/Private/Win32Window.cpp:218-219
        self.params_override: Optional[_abi.vrt_params] = None
        self.DataPath = _abi.PATH_AUTO
        self.Shadows = True
        self.MaxSteps = 255  # Raytracing.hlsl:229
        self.MaxBounces = 2  # MAX_RAY_RECURSION_DEPTH 3 = primary + 2 mirror bounces (RaytracingHlsl.h:32)
        # the reference's artefacts the C++ adaptor reproduces by default (VHipRenderer::ReferenceViewVector / ReferenceBoundaryTexels); this
        # mirror, like the C-ABI, leaves them off unless asked
        self.ReferenceViewVector = False
        self.ReferenceBoundaryTexels = False
        self._env_id = None
        self._tex_ids: Dict[int, int] = {}   # id(image array) -> texture id on the device
        self._tex_keep: Dict[int, np.ndarray] = {}  # keeps the keyed arrays alive so id() stays unique
        self._bound_tex: Dict[int, tuple] = {}  # slot -> the (albedo, normal, rm) texture ids bound to it

    # -- VRenderer surface -------------------------------------------------------------------
    def Start(self) -> bool:
        """VDXRenderer::Start: bring the device up; False (after logging) on failure."""
        if self._ctx:
            return True
        arr = (C.c_int * len(self._devices))(*self._devices)
        rc = self._lib.vrt_create(C.byref(self._ctx), len(self._devices), arr)
        if rc != _abi.VRT_OK:
            print(f"[VHipRenderer] Start failed: {self._lib.vrt_strerror(rc).decode()}")
            self._ctx = C.c_void_p()
            return False
        return True

    def Stop(self) -> None:
        if self._ctx:
            self._lib.vrt_destroy(self._ctx)
            self._ctx = C.c_void_p()
            self._uploaded.clear()
            self._env_id = None
            self._tex_ids.clear()
            self._tex_keep.clear()
            self._bound_tex.clear()

    def IsActive(self) -> bool:
        return bool(self._ctx)

    def SetSceneToRender(self, scene: VScene) -> None:
        self._scene = scene

    def SetRendererMode(self, mode: int) -> None:
        self.RenderMode = int(mode)

    def ResizeRenderOutput(self, width: int, height: int) -> None:
        self.Width, self.Height = int(width), int(height)

    def Render(self) -> np.ndarray:
        """One frame: sync scene → device, march, return the RGBA image [H, W, 4] (float32, or uint8 when
        params_override sets FLAG_OUTPUT_RGBA8)."""
        self._require()
        self.SyncWithScene()
        p = self.make_params()
        out = np.empty((p.height, p.width, 4), dtype=np.uint8 if p.flags & _abi.FLAG_OUTPUT_RGBA8 else np.float32)
        _abi.check(self._lib.vrt_render(self._ctx, C.byref(p), out.ctypes.data_as(C.c_void_p)), "vrt_render")
        return out

    # -- scene mirroring (VRDXScene::SyncWithScene) --------------------------------------------
    def SyncWithScene(self) -> None:
        self._require()
        sc = self._scene
        if sc is None:
            raise RuntimeError("SetSceneToRender was not called")
        vols = sc.volumes()
        # Material textures no volume of the NEW scene names leave the device first — after every slot that still points at one of
        # them has been un-bound (a slot must never name an id the next upload reuses) — so that a scene swap never needs the old
        # and the new texture sets resident together (VRT_MAX_TEXTURES ids in all).
        live = {id(t) for vol in vols for t in vol.Material.textures() if t is not None}
        dead = {self._tex_ids[k] for k in self._tex_ids if k not in live}
        if dead:
            for slot, bound in list(self._bound_tex.items()):
                if any(i in dead for i in bound):
                    _abi.check(self._lib.vrt_volume_set_textures(self._ctx, slot, -1, -1, -1, 100.0, 100.0), "vrt_volume_set_textures")
                    self._bound_tex[slot] = (-1, -1, -1)
            for key in [k for k in self._tex_ids if k not in live]:
                _abi.check(self._lib.vrt_texture_free(self._ctx, self._tex_ids[key]), "vrt_texture_free")
                del self._tex_ids[key]
                del self._tex_keep[key]
        for slot, vol in enumerate(vols):
            if self._uploaded.get(slot) != id(vol) or vol.dirty:
                self.upload_volume(slot, vol)
            else:
                if vol.dirty_box is not None:  # only a box of the resident volume changed
                    self.update_volume_region(slot, vol, *vol.dirty_box)
                # the volume's voxels are unchanged, but its material may name other images or scalars than at the last sync
                # (VMaterial is edited in place; VDXVoxelVolume::UpdateGeometryConstantBuffer, RDXVoxelVolume.cpp:368-397, runs
                # every frame): re-send them — the C-ABI returns at once when nothing differs
                self._bind_material(slot, vol)
        for slot in [s for s in self._uploaded if s >= len(vols)]:
            _abi.check(self._lib.vrt_volume_free(self._ctx, slot), "vrt_volume_free")
            del self._uploaded[slot]
            self._bound_tex.pop(slot, None)
        env = sc.EnvironmentMap
        if env is None:
            if self._env_id is not None:
                _abi.check(self._lib.vrt_env_upload(self._ctx, 0, None), "vrt_env_upload")
                self._env_id = None
        elif self._env_id != id(env):
            e = np.ascontiguousarray(env, dtype=np.uint8)
            if e.ndim != 4 or e.shape[0] != 6 or e.shape[1] != e.shape[2] or e.shape[3] != 4:
                raise ValueError("EnvironmentMap must be uint8 [6, S, S, 4]")
            _abi.check(self._lib.vrt_env_upload(self._ctx, e.shape[1], e.ctypes.data_as(C.c_void_p)), "vrt_env_upload")
            self._env_id = id(env)
        abi_scene = sc.to_abi()
        _abi.check(self._lib.vrt_scene_set(self._ctx, C.byref(abi_scene)), "vrt_scene_set")

    def upload_volume(self, slot: int, vol: VVoxelVolume, as_voxels: bool = False, as_texels: bool = False) -> None:
        """vrt_volume_upload (or _upload_voxels: VVoxel records; or _upload_texels: the reference's own RGBA8 volume
        texture, always the 16-bit format) in the volume's device_format."""
        self._require()
        _abi.check(self._lib.vrt_set_volume_format(self._ctx, int(vol.device_format)), "vrt_set_volume_format")
        if as_texels:
            tex = vol.reference_texels()
            rc = self._lib.vrt_volume_upload_texels(self._ctx, slot, vol.Resolution, vol.VolumeExtends, tex.ctypes.data_as(C.c_void_p))
        elif as_voxels:
            rec = vol.voxel_records()
            rc = self._lib.vrt_volume_upload_voxels(self._ctx, slot, vol.Resolution, vol.VolumeExtends,
                                                    rec.ctypes.data_as(C.c_void_p))
        else:
            d = np.ascontiguousarray(vol.density, dtype=np.float32)
            m = np.ascontiguousarray(vol.material_id, dtype=np.uint8)
            rc = self._lib.vrt_volume_upload(self._ctx, slot, vol.Resolution, vol.VolumeExtends,
                                             d.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p))
        _abi.check(rc, "vrt_volume_upload")
        _abi.check(self._lib.vrt_volume_set_metric(self._ctx, slot, float(vol.density_scale), float(vol.step_max)),
                   "vrt_volume_set_metric")
        self._bind_material(slot, vol)
        self._uploaded[slot] = id(vol)
        vol.dirty = False
        vol.dirty_box = None

    def update_volume_region(self, slot: int, vol: VVoxelVolume, lo, hi) -> None:
        """vrt_volume_update_region: the voxels lo..hi (inclusive xyz corners) of the volume resident in `slot`, from the host
        arrays, in place on the device; every device structure ends as a full upload of the volume would leave it."""
        self._require()
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        d = np.ascontiguousarray(vol.density[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1], dtype=np.float32)
        m = np.ascontiguousarray(vol.material_id[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1], dtype=np.uint8)
        origin = (C.c_int * 3)(x0, y0, z0)
        size = (C.c_int * 3)(x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1)
        _abi.check(self._lib.vrt_volume_update_region(self._ctx, slot, origin, size, d.ctypes.data_as(C.c_void_p),
                                                      m.ctypes.data_as(C.c_void_p)), "vrt_volume_update_region")
        vol.dirty_box = None

    def apply_brushes(self, slot: int, vol: VVoxelVolume, brushes) -> dict:
        """vrt_volume_apply_brushes: the CSG brush records (sphere_brush / box_brush / capsule_brush, at most _abi.MAX_BRUSHES),
        in order, on the volume resident in `slot`, evaluated on the device.  The written box of the host mirror `vol` is then
        read back (download_region) — without touching dirty / dirty_box: the device is already current.  On a TEXEL16 volume the
        mirror receives decoded values (q * 0.01), which quantise again should the volume be uploaded whole later.
        Returns {"written", "lo", "hi"} (xyz, inclusive; lo > hi when nothing was written)."""
        self._require()
        brushes = list(brushes)
        arr = (_abi.vrt_brush * max(1, len(brushes)))(*brushes)
        res = _abi.vrt_brush_result()
        _abi.check(self._lib.vrt_volume_apply_brushes(self._ctx, slot, len(brushes), arr, C.byref(res)), "vrt_volume_apply_brushes")
        lo, hi = tuple(res.lo), tuple(res.hi)
        if res.written and vol is not None:
            self._mirror_box(slot, vol, lo, hi)
        return {"written": int(res.written), "lo": lo, "hi": hi}

    def stamp_volume(self, dst_slot: int, src_slot: int, stamp: _abi.vrt_stamp, vol: Optional[VVoxelVolume] = None) -> dict:
        """vrt_volume_stamp: the volume resident in `src_slot` merged into the one resident in `dst_slot` on the device, as the record
        says (stamp_record / stamp_from_placement): ADD, SUBTRACT or REPLACE of the source's trilinear samples wherever the
        destination's samples land inside the source.  The source slot is only read.  Given the destination's host mirror `vol`, its
        written box is then read back as apply_brushes does.  Returns {"written", "lo", "hi"} (xyz, inclusive; lo > hi when nothing
        was written)."""
        self._require()
        res = _abi.vrt_brush_result()
        _abi.check(self._lib.vrt_volume_stamp(self._ctx, int(dst_slot), int(src_slot), C.byref(stamp), C.byref(res)), "vrt_volume_stamp")
        lo, hi = tuple(res.lo), tuple(res.hi)
        if res.written and vol is not None:
            self._mirror_box(dst_slot, vol, lo, hi)
        return {"written": int(res.written), "lo": lo, "hi": hi}

    def smooth_volume(self, slot: int, smooth: _abi.vrt_smooth, vol: Optional[VVoxelVolume] = None) -> dict:
        """vrt_volume_smooth: the volume resident in `slot` relaxed on the device inside the record's shape (smooth_record): every
        sample there moves towards the mean of its six neighbours, `iterations` times.  Given the slot's host mirror `vol`, the written
        box is then read back as apply_brushes does.  Returns {"written", "lo", "hi"} (xyz, inclusive; lo > hi when nothing was
        written)."""
        self._require()
        res = _abi.vrt_brush_result()
        _abi.check(self._lib.vrt_volume_smooth(self._ctx, int(slot), C.byref(smooth), C.byref(res)), "vrt_volume_smooth")
        lo, hi = tuple(res.lo), tuple(res.hi)
        if res.written and vol is not None:
            self._mirror_box(slot, vol, lo, hi)
        return {"written": int(res.written), "lo": lo, "hi": hi}

    def warp_volume(self, slot: int, warp: _abi.vrt_warp, vol: Optional[VVoxelVolume] = None) -> dict:
        """vrt_volume_warp: the volume resident in `slot` grabbed, twisted, scaled or inflated on the device inside the record's shape
        (warp_record): every sample there takes its value from where the record's motion, faded out by the region's weight, brings it
        from.  Given the slot's host mirror `vol`, the written box is then read back as apply_brushes does.  Returns {"written", "lo",
        "hi"} (xyz, inclusive; lo > hi when nothing was written)."""
        self._require()
        res = _abi.vrt_brush_result()
        _abi.check(self._lib.vrt_volume_warp(self._ctx, int(slot), C.byref(warp), C.byref(res)), "vrt_volume_warp")
        lo, hi = tuple(res.lo), tuple(res.hi)
        if res.written and vol is not None:
            self._mirror_box(slot, vol, lo, hi)
        return {"written": int(res.written), "lo": lo, "hi": hi}

    def _mirror_box(self, slot: int, vol: VVoxelVolume, lo, hi) -> None:
        """The voxels lo..hi of the slot on device 0 into the host mirror `vol` (download_region), dirty / dirty_box untouched."""
        d, m = self.download_region(slot, lo, hi)
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        for name in ("density", "material_id"):
            if not getattr(vol, name).flags.writeable:
                setattr(vol, name, np.array(getattr(vol, name)))
        vol.density[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1] = d
        vol.material_id[x0:x1 + 1, z0:z1 + 1, y0:y1 + 1] = m

    def fill_enclosed(self, slot: int, vol: Optional[VVoxelVolume], wall: float = 1.0, material: int = -1) -> dict:
        """vrt_volume_fill_enclosed: every cavity the volume resident in `slot` encloses (samples with density > 0 that the grid's
        faces cannot reach through 6-neighbour steps over such samples) made solid on the device: -(density + wall), and `material`
        as material id unless it is -1.  wall = 1 and material = 1 suit Voxelizer shells.  Given a host mirror `vol`, its written box
        is then read back as apply_brushes does.  Returns {"filled", "lo", "hi", "sweeps"} (xyz, inclusive; lo > hi when nothing was
        filled)."""
        self._require()
        res = _abi.vrt_fill_result()
        _abi.check(self._lib.vrt_volume_fill_enclosed(self._ctx, slot, float(wall), int(material), C.byref(res)), "vrt_volume_fill_enclosed")
        lo, hi = tuple(res.lo), tuple(res.hi)
        if res.filled and vol is not None:
            self._mirror_box(slot, vol, lo, hi)
        return {"filled": int(res.filled), "lo": lo, "hi": hi, "sweeps": int(res.sweeps)}

    def components(self, slot: int, rec: _abi.vrt_components, vol: Optional[VVoxelVolume] = None, list_capacity: int = 0) -> dict:
        """vrt_volume_components: the 6-connected pieces of the solid samples (density <= 0 or NaN) of the volume resident in `slot`
        labelled on the device, and the ones the record (_abi.components_record) names removed in place.  Given the slot's host
        mirror `vol`, the written box is then read back as apply_brushes does.  Returns _abi.components_dict: the result's fields and
        "list", the first `list_capacity` components by size.  A seed op whose seed has no solid sample around it raises
        _abi.VrtError (ERR_INVALID) and writes nothing."""
        self._require()
        res = _abi.vrt_components_result()
        lst = (_abi.vrt_component * max(int(list_capacity), 1))()
        _abi.check(self._lib.vrt_volume_components(self._ctx, int(slot), C.byref(rec), lst if list_capacity > 0 else None, int(list_capacity),
                                                   C.byref(res)), "vrt_volume_components")
        if res.written and vol is not None:
            self._mirror_box(slot, vol, tuple(res.lo), tuple(res.hi))
        return _abi.components_dict(res, lst)

    def redistance(self, slot: int, vol: Optional[VVoxelVolume], band: int, from_: int = _abi.REDISTANCE_FROM_BOTH, lo=None, hi=None) -> dict:
        """vrt_volume_redistance: the samples lo..hi (inclusive xyz corners; both None: the whole grid) of the volume resident in
        `slot` rewritten on the device as the signed distance, within `band` cells (1..15), to the zero surface of the field the slot
        holds.  from_: _abi.REDISTANCE_FROM_OUTSIDE for Voxelizer shells, filled or not; _FROM_BOTH for true distance fields.  Given a
        host mirror `vol`, the written box is then read back as apply_brushes does.  Returns {"written", "near", "surfels", "lo",
        "hi"}."""
        self._require()
        if (lo is None) != (hi is None):
            raise ValueError("redistance: give both corners of the box or neither")
        res = _abi.vrt_redistance_result()
        origin = size = None
        if lo is not None:
            origin = (C.c_int * 3)(*[int(a) for a in lo])
            size = (C.c_int * 3)(*[int(b) - int(a) + 1 for a, b in zip(lo, hi)])
        _abi.check(self._lib.vrt_volume_redistance(self._ctx, slot, int(band), int(from_), origin, size, C.byref(res)), "vrt_volume_redistance")
        wlo, whi = tuple(res.lo), tuple(res.hi)
        if res.written and vol is not None:
            self._mirror_box(slot, vol, wlo, whi)
        return {"written": int(res.written), "near": int(res.near), "surfels": int(res.surfels), "lo": wlo, "hi": whi}

    def enable_history(self, slot: int, max_entries: int, max_bytes: int) -> None:
        """vrt_volume_history: from now on every edit call on the volume resident in `slot` that changes a bit records, on the
        device, the 4^3 tiles it changed as they were — at most max_entries undo entries and max_bytes bytes per device, the oldest
        entries going first.  (0, 0) turns the history off and frees it.  Uploading over the slot empties the history; freeing the
        slot turns it off."""
        self._require()
        _abi.check(self._lib.vrt_volume_history(self._ctx, int(slot), int(max_entries), int(max_bytes)), "vrt_volume_history")

    def history_info(self, slot: int) -> dict:
        """vrt_volume_history_info: {"enabled", "max_entries", "max_bytes", "undo_entries", "redo_entries", "bytes", "dropped",
        "top_tiles"} — bytes is tiles held x _abi.HISTORY_TILE_BYTES, top_tiles the tiles of the entry undo would take next."""
        self._require()
        info = _abi.vrt_history_info()
        _abi.check(self._lib.vrt_volume_history_info(self._ctx, int(slot), C.byref(info)), "vrt_volume_history_info")
        return {name: int(getattr(info, name)) for name, _ in _abi.vrt_history_info._fields_ if name != "reserved_"}

    def undo(self, slot: int, steps: int = 1, vol: Optional[VVoxelVolume] = None) -> dict:
        """vrt_volume_undo: the `steps` newest recorded edits of the volume resident in `slot` taken back on the device, bit for bit
        (also on a TEXEL16 slot, where a download and an update of the same box are not).  Given the slot's host mirror `vol`, the
        changed box is then read back as apply_brushes does.  Returns {"written", "lo", "hi"} (xyz, inclusive; lo > hi when no
        sample changed); written sums the samples each entry changed."""
        return self._step_history("vrt_volume_undo", slot, steps, vol)

    def redo(self, slot: int, steps: int = 1, vol: Optional[VVoxelVolume] = None) -> dict:
        """vrt_volume_redo: the `steps` edits undone last, done again; otherwise as undo."""
        return self._step_history("vrt_volume_redo", slot, steps, vol)

    def _step_history(self, call: str, slot: int, steps: int, vol: Optional[VVoxelVolume]) -> dict:
        self._require()
        res = _abi.vrt_brush_result()
        _abi.check(getattr(self._lib, call)(self._ctx, int(slot), int(steps), C.byref(res)), call)
        lo, hi = tuple(res.lo), tuple(res.hi)
        if res.written and vol is not None:
            self._mirror_box(slot, vol, lo, hi)
        return {"written": int(res.written), "lo": lo, "hi": hi}

    def mask_apply(self, slot: int, ops) -> dict:
        """vrt_volume_mask_apply: the mask records (_abi.mask_op, at most _abi.MAX_MASK_OPS), in order, on the mask of the volume
        resident in `slot` — protected samples that apply_brushes, stamp_volume, smooth_volume, warp_volume, fill_enclosed, components
        and redistance leave as they were (update_region, undo and redo write through; an upload into the slot drops the mask).  A
        slot without a mask gets an empty one first.  Returns mask_info's dict."""
        self._require()
        ops = list(ops)
        arr = (_abi.vrt_mask_op * max(1, len(ops)))(*ops)
        info = _abi.vrt_mask_info()
        _abi.check(self._lib.vrt_volume_mask_apply(self._ctx, int(slot), len(ops), arr, C.byref(info)), "vrt_volume_mask_apply")
        return _abi.mask_info_dict(info)

    def mask_upload(self, slot: int, mask) -> dict:
        """vrt_volume_mask_upload: the slot's mask from an array indexed [x, z, y] like VVoxelVolume.material_id, non-zero (or True) =
        protected.  Returns mask_info's dict."""
        self._require()
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        _abi.check(self._lib.vrt_volume_mask_upload(self._ctx, int(slot), m.ctypes.data_as(C.c_void_p)), "vrt_volume_mask_upload")
        return self.mask_info(slot)

    def mask_download(self, slot: int, N: int) -> np.ndarray:
        """vrt_volume_mask_download: the mask of the slot (grid size N) on device 0 as a bool array indexed [x, z, y]; all False on a
        slot without a mask."""
        self._require()
        out = np.zeros((int(N),) * 3, np.uint8)
        _abi.check(self._lib.vrt_volume_mask_download(self._ctx, int(slot), out.ctypes.data_as(C.c_void_p)), "vrt_volume_mask_download")
        return out != 0

    def mask_clear(self, slot: int) -> None:
        """vrt_volume_mask_clear: the slot's mask freed on every device; fine on a slot without one."""
        self._require()
        _abi.check(self._lib.vrt_volume_mask_clear(self._ctx, int(slot)), "vrt_volume_mask_clear")

    def mask_info(self, slot: int) -> dict:
        """vrt_volume_mask_info: {"on", "masked", "lo", "hi", "restored"} — the set bits' count and box (xyz, inclusive; lo > hi when
        none), and how many protected samples the latest honouring edit call had changed and got back."""
        self._require()
        info = _abi.vrt_mask_info()
        _abi.check(self._lib.vrt_volume_mask_info(self._ctx, int(slot), C.byref(info)), "vrt_volume_mask_info")
        return _abi.mask_info_dict(info)

    def extract_mesh(self, slot: int, iso: float = 0.0, lo=None, hi=None):
        """vrt_volume_extract_mesh: the surface density = iso of the volume resident in `slot`, over the samples lo..hi (inclusive xyz
        corners; both None: the whole grid), as an indexed triangle mesh built on the device by surface nets: one call that counts,
        one that fetches.  The slot is only read.  Returns (positions (V, 3) float32 in the volume's object space, normals (V, 3)
        float32 pointing outwards, materials (V,) uint8, indices (T, 3) uint32, {"vertices", "quads", "lo", "hi"}) — T = 2 * quads;
        lo / hi: the cells that made a vertex (xyz, inclusive; lo > hi when none)."""
        self._require()
        if (lo is None) != (hi is None):
            raise ValueError("extract_mesh: give both corners of the box or neither")
        origin = size = None
        if lo is not None:
            origin = (C.c_int * 3)(*[int(a) for a in lo])
            size = (C.c_int * 3)(*[int(b) - int(a) + 1 for a, b in zip(lo, hi)])
        res = _abi.vrt_mesh_result()
        call = self._lib.vrt_volume_extract_mesh
        _abi.check(call(self._ctx, slot, float(iso), origin, size, None, None, None, 0, None, 0, C.byref(res)), "vrt_volume_extract_mesh")
        V, Q = int(res.vertices), int(res.quads)
        positions, normals = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
        materials, indices = np.zeros(V, np.uint8), np.zeros((2 * Q, 3), np.uint32)
        if V:
            _abi.check(call(self._ctx, slot, float(iso), origin, size, positions.ctypes.data_as(C.c_void_p), normals.ctypes.data_as(C.c_void_p),
                            materials.ctypes.data_as(C.c_void_p), V, indices.ctypes.data_as(C.c_void_p), 6 * Q, C.byref(res)),
                       "vrt_volume_extract_mesh")
        return positions, normals, materials, indices, {"vertices": V, "quads": Q, "lo": tuple(res.lo), "hi": tuple(res.hi)}

    def measure(self, slot: int, iso: float = 0.0, lo=None, hi=None) -> dict:
        """vrt_volume_measure: how much of the volume resident in `slot` lies at density <= iso, and where, over the samples lo..hi
        (inclusive xyz corners; both None: the whole grid), summed on the device.  The slot is only read.  Returns _abi.measure_dict's
        dict: the record's integer fields ("lo", "hi", "subsamples", "moment1", "moment2", "solid_samples", "active_cells",
        "crossings", "quads", "area_q") and "material_samples" (256 counts); _abi.mass_properties turns it into volume, area,
        centroid and inertia."""
        self._require()
        if (lo is None) != (hi is None):
            raise ValueError("measure: give both corners of the box or neither")
        origin = size = None
        if lo is not None:
            origin = (C.c_int * 3)(*[int(a) for a in lo])
            size = (C.c_int * 3)(*[int(b) - int(a) + 1 for a, b in zip(lo, hi)])
        res, counts = _abi.vrt_measure_result(), (C.c_uint64 * 256)()
        _abi.check(self._lib.vrt_volume_measure(self._ctx, slot, float(iso), origin, size, C.byref(res), counts), "vrt_volume_measure")
        return _abi.measure_dict(res, counts)

    def download_region(self, slot: int, lo, hi):
        """vrt_volume_download_region: the voxels lo..hi (inclusive xyz corners) of the slot on device 0 as (density float32,
        material uint8), both indexed [x, z, y] like VVoxelVolume.density; a TEXEL16 slot decodes like download_volume."""
        self._require()
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        sx, sy, sz = x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1
        rec = np.zeros(max(0, sx) * max(0, sy) * max(0, sz), dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        _abi.check(self._lib.vrt_volume_download_region(self._ctx, slot, (C.c_int * 3)(x0, y0, z0), (C.c_int * 3)(sx, sy, sz),
                                                        rec.ctypes.data_as(C.c_void_p)), "vrt_volume_download_region")
        shape = (sx, sz, sy)
        return np.ascontiguousarray(rec["density"].reshape(shape)), np.ascontiguousarray(rec["material"].reshape(shape))

    def _bind_material(self, slot: int, vol: VVoxelVolume) -> None:
        """The slot's material scalars and texture bindings as the volume's VMaterial holds them NOW (images uploaded on first
        sight).  Both C-ABI calls return without touching the device when nothing changed."""
        mat = vol.Material.to_abi()
        _abi.check(self._lib.vrt_volume_set_material(self._ctx, slot, C.byref(mat)), "vrt_volume_set_material")
        ids = [self.upload_texture(t) if t is not None else -1 for t in vol.Material.textures()]
        _abi.check(self._lib.vrt_volume_set_textures(self._ctx, slot, ids[0], ids[1], ids[2], float(vol.Material.TextureScale[0]),
                                                     float(vol.Material.TextureScale[1])), "vrt_volume_set_textures")
        self._bound_tex[slot] = tuple(ids)

    def set_palette(self, slot: int, entries) -> None:
        """vrt_volume_set_palette: per-voxel materials for the slot.  entries: a sequence of (tint4, roughness, metallic), or an (n, 6)
        array of rows (r, g, b, a, roughness, metallic), n in 1..256; empty or None takes the palette away.  A hit then renders with the
        entry of the material id of the voxel it lands on (the rule: vrt.h); ids beyond the palette keep the slot's own material."""
        self._require()
        rows = []
        if entries is not None:
            if isinstance(entries, np.ndarray):
                rows = [tuple(float(x) for x in r) for r in np.asarray(entries, dtype=np.float32).reshape(-1, 6)]
            else:
                rows = [tuple(float(x) for x in tint) + (float(rough), float(metal)) for tint, rough, metal in entries]
        arr = (_abi.vrt_material * max(len(rows), 1))()
        for m, r in zip(arr, rows):
            m.tint[:] = r[:4]
            m.roughness, m.metallic = r[4], r[5]
        _abi.check(self._lib.vrt_volume_set_palette(self._ctx, slot, len(rows), arr if rows else None), "vrt_volume_set_palette")

    def get_palette(self, slot: int) -> np.ndarray:
        """vrt_volume_get_palette: the slot's palette as an (n, 6) float32 array of rows (r, g, b, a, roughness, metallic), bit for bit
        what set_palette was given; n == 0 without a palette."""
        self._require()
        arr = (_abi.vrt_material * _abi.VRT_MAX_PALETTE)()
        n = C.c_int(0)
        _abi.check(self._lib.vrt_volume_get_palette(self._ctx, slot, _abi.VRT_MAX_PALETTE, arr, C.byref(n)), "vrt_volume_get_palette")
        return np.array([list(m.tint) + [m.roughness, m.metallic] for m in arr[:n.value]], dtype=np.float32).reshape(-1, 6)

    def voxelize_mesh(self, slot: int, positions: np.ndarray, indices: np.ndarray, resolution: int, extent: float) -> int:
        """The Voxelizer's hot loop on the device (vrt_voxelize_mesh): fills `slot` with the shell field of a
        triangle mesh given in volume space; returns the number of skipped (degenerate) triangles.  The slot is
        not tracked by SyncWithScene: pair it with download_volume() or instance it through a raw vrt_scene."""
        self._require()
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        skipped = C.c_size_t(0)
        _abi.check(self._lib.vrt_voxelize_mesh(self._ctx, slot, resolution, float(extent), pos.ctypes.data_as(C.c_void_p), len(pos),
                                               idx.ctypes.data_as(C.c_void_p), len(idx), C.byref(skipped)), "vrt_voxelize_mesh")
        self._uploaded.pop(slot, None)
        return int(skipped.value)

    def download_volume(self, slot: int, resolution: int, extent: float) -> VVoxelVolume:
        """vrt_volume_download: the slot as a VVoxelVolume (densities + materials)."""
        self._require()
        vol = VVoxelVolume(resolution, extent)
        rec = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        _abi.check(self._lib.vrt_volume_download(self._ctx, slot, rec.ctypes.data_as(C.c_void_p)), "vrt_volume_download")
        vol.density = np.ascontiguousarray(rec["density"].reshape(vol.N, vol.N, vol.N))
        vol.material_id = np.ascontiguousarray(rec["material"].reshape(vol.N, vol.N, vol.N))
        return vol

    def upload_texture(self, image: np.ndarray) -> int:
        """VRenderer::InitializeTexture + UploadToGPU for a 2D material texture (uint8 [H, W, 4]); images are
        shared between volumes by identity, like the reference's path-keyed texture table (RDXScene.cpp:905-925)."""
        self._require()
        key = id(image)
        if key in self._tex_ids:
            return self._tex_ids[key]
        used = set(self._tex_ids.values())
        tid = next((i for i in range(_abi.VRT_MAX_TEXTURES) if i not in used), None)
        if tid is None:
            raise RuntimeError("too many material textures")
        img = np.ascontiguousarray(image, dtype=np.uint8)
        _abi.check(self._lib.vrt_texture_upload(self._ctx, tid, img.shape[1], img.shape[0], img.ctypes.data_as(C.c_void_p)),
                   "vrt_texture_upload")
        self._tex_ids[key] = tid
        self._tex_keep[key] = image
        return tid

    # -- parameters / raw launches ---------------------------------------------------------------
    def make_params(self) -> _abi.vrt_params:
        if self.params_override is not None:
            p = _abi.vrt_params.from_buffer_copy(self.params_override)
        else:
            cell = min((v.GetCellSize() for v in self._scene.volumes()), default=1.0) if self._scene else 1.0
            res = max((v.Resolution for v in self._scene.volumes()), default=0) if self._scene else 0
            p = default_params(self.Width, self.Height, cell, max_steps=march_budget(res, self.MaxSteps), shadow=self.Shadows)
            p.max_bounces = self.MaxBounces
            if self.ReferenceViewVector:
                p.flags |= _abi.FLAG_REFERENCE_VIEW_VECTOR
            if self.ReferenceBoundaryTexels:
                p.flags |= _abi.FLAG_REFERENCE_BOUNDARY_TEXELS
        p.width, p.height = self.Width, self.Height
        p.mode = self.RenderMode
        if self.params_override is None:
            p.path = self.DataPath
        return p

    def render_rows(self, params: _abi.vrt_params, row0: int, rows: int, device_ptr: int, stream: int = 0) -> None:
        """Asynchronous tile render into caller-owned device memory (vrt_render_rows)."""
        self._require()
        _abi.check(self._lib.vrt_render_rows(self._ctx, C.byref(params), row0, rows, C.c_void_p(device_ptr),
                                             C.c_void_p(stream)), "vrt_render_rows")

    def render_strips(self, params: _abi.vrt_params, strip_rows: int, first_strip: int, strip_stride: int, n_strips: int,
                      device_ptr: int, stream: int = 0) -> None:
        """Asynchronous render of interleaved strips into a compact device tile (vrt_render_strips)."""
        self._require()
        _abi.check(self._lib.vrt_render_strips(self._ctx, C.byref(params), strip_rows, first_strip, strip_stride, n_strips,
                                               C.c_void_p(device_ptr), C.c_void_p(stream)), "vrt_render_strips")

    def render_block(self, params: _abi.vrt_params, n_frames: int, device_ptr: int, frame_stride_bytes: int, stream: int = 0,
                     strips=None, rows=None, cameras=None, scenes=None) -> None:
        """vrt_render_block: n_frames frames of the current scene in flight with one call, frame f into
        device_ptr + f*frame_stride_bytes; to the caller one asynchronous operation on `stream`.  strips = (strip_rows,
        first_strip, strip_stride, n_strips) or rows = (row0, rows) (default: the whole frame); cameras: n_frames
        (position[3], rotation[4], fov_deg) triples overriding the scene's camera per frame; scenes: per-frame scene state —
        (a ctypes vrt_scene array from scene_array(), index of the first scene): frame f renders scenes[start + f] (objects,
        lights and camera that move from frame to frame) over the volumes of the scene this renderer is synced with."""
        self._require()
        b = _abi.vrt_block()
        b.n_frames = int(n_frames)
        if strips is not None:
            b.strip_rows, b.first_strip, b.strip_stride, b.n_strips = (int(x) for x in strips)
        else:
            b.row0, b.rows = (int(x) for x in rows) if rows is not None else (0, int(params.height))
        if cameras is not None:
            # a list of (position, rotation, fov) triples, or (a ctypes array from camera_array(), index of the first camera)
            arr, start = cameras if isinstance(cameras, tuple) and isinstance(cameras[0], C.Array) else (self.camera_array(cameras), 0)
            if start < 0 or start + b.n_frames > len(arr):
                raise ValueError("camera range outside the array")
            b.cameras = C.cast(C.byref(arr, start * C.sizeof(_abi.vrt_camera)), C.POINTER(_abi.vrt_camera))
        if scenes is not None:
            sarr, sstart = scenes
            if sstart < 0 or sstart + b.n_frames > len(sarr):
                raise ValueError("scene range outside the array")
            b.scenes = C.cast(C.byref(sarr, sstart * C.sizeof(_abi.vrt_scene)), C.POINTER(_abi.vrt_scene))
        b.frame_stride_bytes = int(frame_stride_bytes)
        _abi.check(self._lib.vrt_render_block(self._ctx, C.byref(params), C.byref(b), C.c_void_p(device_ptr), C.c_void_p(stream)),
                   "vrt_render_block")

    def scene_array(self, scenes):
        """A ctypes vrt_scene array from VScene objects that place (a subset of) the SAME volumes as the scene this renderer
        is synced with (SetSceneToRender + SyncWithScene): their instances name the synced scene's volume slots.  For
        render_block(scenes=(array, start)): objects, lights and camera per frame."""
        if self._scene is None:
            raise RuntimeError("SetSceneToRender was not called")
        slots = {id(vol): i for i, vol in enumerate(self._scene.volumes())}
        arr = (_abi.vrt_scene * len(scenes))()
        for k, sc in enumerate(scenes):
            a = sc.to_abi()
            own = sc.volumes()
            for i in range(a.n_instances):
                vol = own[a.instances[i].volume_slot]
                if id(vol) not in slots:
                    raise ValueError("a per-frame scene places a volume the synced scene does not hold")
                a.instances[i].volume_slot = slots[id(vol)]
            arr[k] = a
        return arr

    @staticmethod
    def camera_array(cameras):
        """A ctypes vrt_camera array from (position[3], rotation[4], fov_deg) triples, to be passed (with a start index) to
        render_block many times without rebuilding it."""
        arr = (_abi.vrt_camera * len(cameras))()
        for c, (pos, rot, fov) in zip(arr, cameras):
            c.position[:] = [float(x) for x in pos]
            c.rotation[:] = [float(x) for x in rot]
            c.fov_deg = float(fov)
        return arr

    def render_begin(self, slot: int, params: Optional[_abi.vrt_params] = None) -> _abi.vrt_params:
        """vrt_render_begin: sync the scene, snapshot it and enqueue the whole frame on frame slot `slot`
        (0..VRT_FRAMES_IN_FLIGHT-1); returns at once.  Collect with render_end(slot, params)."""
        self._require()
        self.SyncWithScene()
        p = params if params is not None else self.make_params()
        _abi.check(self._lib.vrt_render_begin(self._ctx, C.byref(p), slot), "vrt_render_begin")
        return p

    def render_end(self, slot: int, params: _abi.vrt_params, copy: bool = True) -> Optional[np.ndarray]:
        """vrt_render_end: wait for the frame begun on `slot` and return a copy of its pixels (copy=False: just wait;
        the pixels stay in the slot's pinned host frame)."""
        self._require()
        ptr = C.c_void_p()
        _abi.check(self._lib.vrt_render_end(self._ctx, slot, C.byref(ptr)), "vrt_render_end")
        if not copy:
            return None
        if params.flags & _abi.FLAG_OUTPUT_RGBA8:
            buf = (C.c_uint8 * (params.width * params.height * 4)).from_address(ptr.value)
            return np.frombuffer(buf, dtype=np.uint8).reshape(params.height, params.width, 4).copy()
        buf = (C.c_float * (params.width * params.height * 4)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.float32).reshape(params.height, params.width, 4).copy()

    # -- ray queries (vrt_trace_rays*, vrt_camera_rays) ----------------------------------------------------------------------------
    def trace_rays(self, origins, directions, t_max=10000.0, any_hit: bool = False, params: Optional[_abi.vrt_params] = None) -> dict:
        """Closest hit (or, any_hit, occlusion within t_max) of world-space rays against the synced scene, on the GPU
        (vrt_trace_rays_host): a dict of numpy arrays hit, t, normal, instance, voxel, material, steps.  Syncs the scene first;
        params defaults to make_params() (the render's march contract).  t_max: a scalar or one value per ray."""
        self._require()
        self.SyncWithScene()
        p = params if params is not None else self.make_params()
        rays = make_rays(origins, directions, t_max)
        hits = np.zeros(len(rays), HIT_DTYPE)
        query = _abi.QUERY_ANY if any_hit else _abi.QUERY_CLOSEST
        _abi.check(self._lib.vrt_trace_rays_host(self._ctx, C.byref(p), query, len(rays), rays.ctypes.data_as(C.c_void_p),
                                                 hits.ctypes.data_as(C.c_void_p)), "vrt_trace_rays_host")
        return hits_to_dict(hits)

    def trace_rays_device(self, params: _abi.vrt_params, query: int, n: int, rays_ptr: int, hits_ptr: int, stream: int = 0) -> None:
        """Asynchronous query of n vrt_ray records in device memory into n vrt_hit records (vrt_trace_rays); allocates
        nothing, so it can be captured into a graph.  Does not sync the scene."""
        self._require()
        _abi.check(self._lib.vrt_trace_rays(self._ctx, C.byref(params), int(query), int(n), C.c_void_p(rays_ptr), C.c_void_p(hits_ptr),
                                            C.c_void_p(stream)), "vrt_trace_rays")

    def camera_rays(self, pixels, width: Optional[int] = None, height: Optional[int] = None) -> np.ndarray:
        """The march kernel's camera rays of (x, y) pixels of the scene's camera, bit for bit, as a vrt_ray array
        (vrt_camera_rays; host only).  Default frame size: the current output size."""
        if self._scene is None:
            raise RuntimeError("SetSceneToRender was not called")
        px = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        rays = np.zeros(len(px), RAY_DTYPE)
        sc = self._scene.to_abi()
        _abi.check(self._lib.vrt_camera_rays(C.byref(sc), int(width or self.Width), int(height or self.Height), len(px),
                                             px.ctypes.data_as(C.c_void_p), rays.ctypes.data_as(C.c_void_p)), "vrt_camera_rays")
        return rays

    def pick(self, px: int, py: int, params: Optional[_abi.vrt_params] = None) -> dict:
        """What lies under pixel (px, py) of the current output size: the closest hit of its camera ray with make_params()
        (the render's cone_eps), as trace_rays returns it for one ray, with scalar fields."""
        r = self.camera_rays([(px, py)])
        out = self.trace_rays(r["origin"], r["direction"], r["t_max"], params=params)
        return {k: (v[0] if v.ndim == 1 else v[0].copy()) for k, v in out.items()}

    # -- distance queries (vrt_query_points*) -------------------------------------------------------------------------------------------
    def query_points(self, points, iterations: int = 0, tolerance: float = 0.0) -> dict:
        """How far world-space points are from the nearest surface of the synced scene, and in which direction, on the GPU
        (vrt_query_points_host): a dict of numpy arrays distance, normal, instance, voxel, material, sampled, moves, position.
        iterations > 0 moves every point onto the surface first (project_points).  Syncs the scene first."""
        self._require()
        self.SyncWithScene()
        pts = make_points(points)
        res = np.zeros(len(pts), POINT_RESULT_DTYPE)
        _abi.check(self._lib.vrt_query_points_host(self._ctx, int(iterations), float(tolerance), len(pts), pts.ctypes.data_as(C.c_void_p),
                                                   res.ctypes.data_as(C.c_void_p)), "vrt_query_points_host")
        return point_results_to_dict(res)

    def query_points_device(self, iterations: int, tolerance: float, n: int, points_ptr: int, results_ptr: int, stream: int = 0) -> None:
        """Asynchronous query of n vrt_point records in device memory into n vrt_point_result records (vrt_query_points);
        allocates nothing, so it can be captured into a graph.  Does not sync the scene."""
        self._require()
        _abi.check(self._lib.vrt_query_points(self._ctx, int(iterations), float(tolerance), int(n), C.c_void_p(points_ptr),
                                              C.c_void_p(results_ptr), C.c_void_p(stream)), "vrt_query_points")

    def project_points(self, points, iterations: int = 8, tolerance: float = 1e-4) -> dict:
        """The points moved onto the nearest surface: up to `iterations` moves of p - normal * distance, stopping within `tolerance`
        (world units) of it; the records of the moved points, `position` being where they ended."""
        return self.query_points(points, iterations=iterations, tolerance=tolerance)

    # -- sweep queries (vrt_query_sweeps*) ------------------------------------------------------------------------------------------------
    def sweep_spheres(self, origins, directions, radius=0.0, t_max=10000.0, max_steps: int = 256, tolerance: float = 1e-3,
                      step_min: float = 1e-3) -> dict:
        """Where spheres of `radius`, their centres moved from `origins` along `directions` for at most `t_max`, first touch the synced
        scene, on the GPU (vrt_query_sweeps_host): a dict of numpy arrays t, normal, instance, voxel, material, flags, steps, distance,
        position, hit, exhausted, initial.  tolerance and step_min are world units.  Syncs the scene first."""
        self._require()
        self.SyncWithScene()
        rec = make_sweeps(origins, directions, radius, t_max)
        res = np.zeros(len(rec), SWEEP_HIT_DTYPE)
        _abi.check(self._lib.vrt_query_sweeps_host(self._ctx, int(max_steps), float(tolerance), float(step_min), len(rec),
                                                   rec.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)), "vrt_query_sweeps_host")
        return sweep_hits_to_dict(res)

    def sweep_spheres_device(self, max_steps: int, tolerance: float, step_min: float, n: int, sweeps_ptr: int, hits_ptr: int,
                             stream: int = 0) -> None:
        """Asynchronous sweep of n vrt_sweep records in device memory into n vrt_sweep_hit records (vrt_query_sweeps); allocates
        nothing, so it can be captured into a graph.  Does not sync the scene."""
        self._require()
        _abi.check(self._lib.vrt_query_sweeps(self._ctx, int(max_steps), float(tolerance), float(step_min), int(n), C.c_void_p(sweeps_ptr),
                                              C.c_void_p(hits_ptr), C.c_void_p(stream)), "vrt_query_sweeps")

    # -- contact queries (vrt_query_contacts) ----------------------------------------------------------------------------------------
    def query_contacts(self, a: int, b: int, margin: float = 0.0) -> dict:
        """Where the surface of instance `a` of the synced scene touches or enters instance `b`, on the GPU (vrt_query_contacts: counted,
        then fetched): the points of a's surface whose distance to b's surface is <= margin (world units), in the order of a's cells.  A
        dict of numpy arrays position, distance, normal, material_a, normal_a, material_b, cell_a, with the result's lo, hi, contacts,
        candidates and min_distance.  One-sided: swap a and b for b's surface in a.  Syncs the scene first."""
        self._require()
        self.SyncWithScene()
        res = _abi.vrt_contacts_result()
        call = self._lib.vrt_query_contacts
        _abi.check(call(self._ctx, int(a), int(b), float(margin), None, 0, C.byref(res)), "vrt_query_contacts")
        rec = np.zeros(int(res.contacts), CONTACT_DTYPE)
        if len(rec):
            _abi.check(call(self._ctx, int(a), int(b), float(margin), rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(res)), "vrt_query_contacts")
        return contacts_to_dict(rec, res)

    # -- multi-GPU exchange, one process per GPU (vrt_comm_* / vrt_gather_tiles: RCCL ncclGather) --------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the 128-byte communicator id to hand to every rank (vrt_comm_unique_id)."""
        buf = (C.c_uint8 * _abi.VRT_COMM_ID_BYTES)()
        _abi.check(_abi.load().vrt_comm_unique_id(buf), "vrt_comm_unique_id")
        return bytes(buf)

    def comm_init(self, world: int, rank: int, unique_id: bytes) -> None:
        """Every rank (collective): join the communicator of `unique_id` on this renderer's device."""
        self._require()
        if len(unique_id) != _abi.VRT_COMM_ID_BYTES:
            raise ValueError("unique_id must be VRT_COMM_ID_BYTES long")
        buf = (C.c_uint8 * _abi.VRT_COMM_ID_BYTES).from_buffer_copy(unique_id)
        _abi.check(self._lib.vrt_comm_init(self._ctx, int(world), int(rank), buf), "vrt_comm_init")

    def comm_expect_sizes(self, gather_tile_bytes: int, exchange_chunk_bytes: int) -> None:
        """Every rank (collective, synchronous): agree on the byte counts gather_tiles / exchange_tiles are going to be called with;
        a rank that disagrees makes the call fail on every rank instead of hanging the collective later."""
        self._require()
        _abi.check(self._lib.vrt_comm_expect_sizes(self._ctx, int(gather_tile_bytes), int(exchange_chunk_bytes)), "vrt_comm_expect_sizes")

    def gather_tiles(self, tile_ptr: int, frame_ptr: int, tile_bytes: int, root: int = 0, stream: int = 0) -> None:
        """Asynchronous ncclGather of this rank's device tile into rank `root`'s device frame (rank-major)."""
        self._require()
        _abi.check(self._lib.vrt_gather_tiles(self._ctx, C.c_void_p(tile_ptr), C.c_void_p(frame_ptr) if frame_ptr else None, int(tile_bytes),
                                              int(root), C.c_void_p(stream)), "vrt_gather_tiles")

    def exchange_tiles(self, tiles_ptr: int, recv_ptr: int, chunk_bytes: int, stream: int = 0) -> None:
        """Asynchronous all-to-all of equal chunks (vrt_exchange_tiles): chunk d of `tiles_ptr` goes to rank d, chunk s of
        `recv_ptr` comes from rank s."""
        self._require()
        _abi.check(self._lib.vrt_exchange_tiles(self._ctx, C.c_void_p(tiles_ptr), C.c_void_p(recv_ptr), int(chunk_bytes), C.c_void_p(stream)),
                   "vrt_exchange_tiles")

    def last_timing(self) -> dict:
        self._require()
        t = _abi.vrt_timing()
        _abi.check(self._lib.vrt_last_timing(self._ctx, C.byref(t)), "vrt_last_timing")
        return {name: getattr(t, name) for name, _ in t._fields_}

    def timing_history(self, n: int) -> List[float]:
        self._require()
        buf = (C.c_float * max(n, 1))()
        m = self._lib.vrt_timing_history(self._ctx, n, buf)
        if m < 0:
            _abi.check(m, "vrt_timing_history")
        return [buf[i] for i in range(m)]

    def launch_history(self, n: int):
        """(kernel ms, frames covered) of the last n march launches, oldest first (vrt_launch_history); 0 ms = not event-timed."""
        self._require()
        ms = (C.c_float * max(n, 1))()
        fr = (C.c_int * max(n, 1))()
        m = self._lib.vrt_launch_history(self._ctx, n, ms, fr)
        if m < 0:
            _abi.check(m, "vrt_launch_history")
        return [(ms[i], fr[i]) for i in range(m)]

    def gather_ceiling(self, fmt: int = _abi.FORMAT_F32, coherent_lanes: bool = False, n_bricks: int = 32) -> float:
        """G trilinear samples per second the chip sustains for the march's inner operation in isolation (vrt_debug_gather_ceiling)."""
        self._require()
        out = C.c_float()
        _abi.check(self._lib.vrt_debug_gather_ceiling(self._ctx, int(fmt), 1 if coherent_lanes else 0, int(n_bricks), C.byref(out)), "vrt_debug_gather_ceiling")
        return float(out.value)

    def last_kernel_form(self) -> int:
        """Bit set of _abi.FORM_* naming the closest-hit kernel form the last march launch ran (vrt_debug_last_kernel_form)."""
        self._require()
        f = self._lib.vrt_debug_last_kernel_form(self._ctx)
        if f < 0:
            _abi.check(f, "vrt_debug_last_kernel_form")
        return int(f)

    def wave_records(self, which: int = 0) -> np.ndarray:
        """Per-wave records of the last launch, [waves, 8] uint32 (vrt_debug_wave_records):
        which=0 counters, which=1 diagnostic timeline (after a FLAG_DIAG_TIMELINE launch)."""
        self._require()
        n = self._lib.vrt_debug_wave_records(self._ctx, which, None, 0)
        if n < 0:
            _abi.check(int(n), "vrt_debug_wave_records")
        buf = np.zeros(int(n), dtype=np.uint32)
        self._lib.vrt_debug_wave_records(self._ctx, which, buf.ctypes.data_as(C.c_void_p), int(n))
        return buf.reshape(-1, 8)

    def _require(self) -> None:
        if not self._ctx:
            raise RuntimeError("renderer is not active (Start() not called or failed)")

    def __enter__(self):
        if not self.Start():
            raise RuntimeError("VHipRenderer.Start() failed — no HIP device or library error")
        return self

    def __exit__(self, *exc):
        self.Stop()
        return False


def algorithmic_bytes(t: dict, bytes_per_pixel: int = 16) -> int:
    """32 B per trilinear sample, 6 samples per hit normal, one framebuffer store per pixel
    rendered (= primary ray)."""
    samples = t["primary_steps"] + t["shadow_steps"]
    return 32 * samples + 32 * 6 * t["hits"] + bytes_per_pixel * t["primary_rays"]
