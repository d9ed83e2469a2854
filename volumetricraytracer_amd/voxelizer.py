"""ctypes access to the C++ Voxelizer (csrc/host, libvrt_host.so) plus small mesh / glTF helpers
used by tests and bench.py.  The conversion itself is the C++ restatement of the reference's
Voxelizer (VolumeConverter.cpp); nothing is voxelized in Python."""
from __future__ import annotations

import base64
import ctypes as C
import json
import math
import os
import struct
from typing import Tuple

import numpy as np

from . import _abi
from .scene import VMaterial, VVoxelVolume

HOST_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libvrt_host.so")
_host = None


def load_host() -> C.CDLL:
    global _host
    if _host is None:
        path = os.environ.get("VRT_HOST_LIB") or HOST_LIB_PATH  # VRT_HOST_LIB: the sanitizer build (make -C csrc/host asan)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run __graft_entry__.build()")
        _abi.load()  # libvrt_host.so links libvrt_hip.so: settle the HIP runtime first
        lib = C.CDLL(path)
        lib.vrh_last_error.restype = C.c_char_p
        lib.vrh_convert_mesh.restype = C.c_void_p
        lib.vrh_convert_mesh.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.c_char_p]
        lib.vrh_volume_info.restype = C.c_int
        lib.vrh_volume_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_float)] * 4
        lib.vrh_volume_copy_voxels.restype = C.c_int
        lib.vrh_volume_copy_voxels.argtypes = [C.c_void_p, C.c_void_p]
        lib.vrh_volume_free.restype = None
        lib.vrh_volume_free.argtypes = [C.c_void_p]
        lib.vrh_voxelize_file.restype = C.c_int
        lib.vrh_voxelize_file.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
        lib.vrh_fill_enclosed.restype = C.c_int
        lib.vrh_fill_enclosed.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.POINTER(_abi.vrt_fill_result)]
        lib.vrh_redistance.restype = C.c_int
        lib.vrh_redistance.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(_abi.vrt_redistance_result)]
        lib.vrh_stamp.restype = C.c_int
        lib.vrh_stamp.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int,
                                  C.POINTER(_abi.vrt_stamp), C.POINTER(_abi.vrt_brush_result)]
        lib.vrh_warp.restype = C.c_int
        lib.vrh_warp.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(_abi.vrt_warp), C.POINTER(_abi.vrt_brush_result)]
        lib.vrh_smooth.restype = C.c_int
        lib.vrh_smooth.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(_abi.vrt_smooth), C.POINTER(_abi.vrt_brush_result)]
        lib.vrh_components.restype = C.c_int
        lib.vrh_components.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.vrt_components), C.POINTER(_abi.vrt_component), C.c_int,
                                       C.POINTER(_abi.vrt_components_result)]
        lib.vrh_mask_apply.restype = C.c_int
        lib.vrh_mask_apply.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(_abi.vrt_mask_op), C.POINTER(_abi.vrt_mask_info)]
        lib.vrh_extract_mesh.restype = C.c_int
        lib.vrh_extract_mesh.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(_abi.vrt_mesh_result)]
        lib.vrh_contacts.restype = C.c_int
        lib.vrh_contacts.argtypes = [C.POINTER(vrh_placed_volume), C.POINTER(vrh_placed_volume), C.c_float, C.c_int, C.c_void_p, C.c_size_t,
                                     C.POINTER(_abi.vrt_contacts_result)]
        lib.vrh_measure.restype = C.c_int
        lib.vrh_measure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(_abi.vrt_measure_result), C.POINTER(C.c_uint64)]
        lib.vrh_gltf_mesh.restype = C.c_int
        lib.vrh_gltf_mesh.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.vrh_vox_rewrite.restype = C.c_int
        lib.vrh_vox_rewrite.argtypes = [C.c_char_p, C.c_char_p]
        _host = lib
    return _host


def convert_mesh(positions: np.ndarray, indices: np.ndarray, bounds_extends, mesh_name: str,
                 material: VMaterial | None = None) -> VVoxelVolume:
    """VVolumeConverter::ConvertMeshInfoToVoxelVolume on arrays that are already in the importer's
    output space (positions x100 and re-centred, bounds = half size + 5)."""
    lib = load_host()
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    be = (C.c_float * 3)(*[float(x) for x in bounds_extends])
    h = lib.vrh_convert_mesh(pos.ctypes.data, len(pos), idx.ctypes.data, len(idx), be, mesh_name.encode())
    if not h:
        raise RuntimeError("vrh_convert_mesh: " + lib.vrh_last_error().decode(errors="replace"))
    try:
        res, size = C.c_int(), C.c_int()
        ext, cell, scale, smax = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        lib.vrh_volume_info(h, C.byref(res), C.byref(size), C.byref(ext), C.byref(cell), C.byref(scale), C.byref(smax))
        vol = VVoxelVolume(res.value, ext.value)
        rec = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        lib.vrh_volume_copy_voxels(h, rec.ctypes.data)
        vol.density = np.ascontiguousarray(rec["density"].reshape(vol.N, vol.N, vol.N))
        vol.material_id = np.ascontiguousarray(rec["material"].reshape(vol.N, vol.N, vol.N))
        vol.density_scale = scale.value
        vol.step_max = smax.value
        if material is not None:
            vol.Material = material
        return vol
    finally:
        lib.vrh_volume_free(h)


def fill_enclosed_host(vol: VVoxelVolume, wall: float = 1.0, material: int = -1) -> dict:
    """VVolumeConverter::FillEnclosed (the host build of vrt_volume_fill_enclosed's rule) on a volume's densities and material ids, in
    place: every sample with density > 0 that a 6-connected flood from the grid's faces over such samples does not reach gets
    -(density + wall) and, unless material is -1, that material id.  Returns {"filled", "lo", "hi"} (xyz, inclusive; lo > hi when
    nothing was filled)."""
    lib = load_host()
    rec = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
    rec["density"] = np.asarray(vol.density, np.float32).reshape(-1)
    rec["material"] = np.asarray(vol.material_id, np.uint8).reshape(-1)
    res = _abi.vrt_fill_result()
    if lib.vrh_fill_enclosed(rec.ctypes.data, vol.N, float(wall), int(material), C.byref(res)) != 0:
        raise RuntimeError("vrh_fill_enclosed: " + lib.vrh_last_error().decode(errors="replace"))
    if res.filled:
        vol.density = np.ascontiguousarray(rec["density"].reshape(vol.N, vol.N, vol.N))
        vol.material_id = np.ascontiguousarray(rec["material"].reshape(vol.N, vol.N, vol.N))
        vol.dirty = True
    return {"filled": int(res.filled), "lo": tuple(res.lo), "hi": tuple(res.hi)}


def components_host(vol: VVoxelVolume, rec: _abi.vrt_components, texel16: bool = False, list_capacity: int = 0) -> dict:
    """VVolumeConverter::Components (the host build of vrt_volume_components's rule) on a volume's densities and material ids, in place.
    texel16: the densities are the integer field +-q of a TEXEL16 slot.  Raises _abi.VrtError with the code vrt_volume_components
    returns for a record it refuses or a seed without a solid sample around it.  Returns _abi.components_dict."""
    lib = load_host()
    buf = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
    buf["density"] = np.asarray(vol.density, np.float32).reshape(-1)
    buf["material"] = np.asarray(vol.material_id, np.uint8).reshape(-1)
    res = _abi.vrt_components_result()
    lst = (_abi.vrt_component * max(int(list_capacity), 1))()
    rc = lib.vrh_components(buf.ctypes.data, vol.N, int(bool(texel16)), C.byref(rec), lst if list_capacity > 0 else None, int(list_capacity),
                            C.byref(res))
    _abi.check(rc, "vrh_components")
    if res.written:
        vol.density = np.ascontiguousarray(buf["density"].reshape(vol.N, vol.N, vol.N))
        vol.material_id = np.ascontiguousarray(buf["material"].reshape(vol.N, vol.N, vol.N))
        vol.dirty = True
    return _abi.components_dict(res, lst)


def redistance_host(vol: VVoxelVolume, band: int, from_: int = _abi.REDISTANCE_FROM_BOTH, lo=None, hi=None, unit=None, texel16: bool = False) -> dict:
    """VVolumeConverter::Redistance (the host build of vrt_volume_redistance's rule) on a volume's densities, in place: the samples
    lo..hi (inclusive xyz corners; both None: the whole grid) become the signed distance, within `band` cells, to the zero surface of
    the field.  unit: density units per cell, by default cell / density_scale in float32 as the device computes it; texel16: the
    densities are the integer field +-q of a TEXEL16 slot.  Material ids stay.  Returns {"written", "near", "surfels", "lo", "hi"}."""
    lib = load_host()
    if (lo is None) != (hi is None):
        raise ValueError("redistance_host: give both corners of the box or neither")
    rec = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
    rec["density"] = np.asarray(vol.density, np.float32).reshape(-1)
    if unit is None:
        unit = np.float32(vol.GetCellSize()) / np.float32(vol.density_scale)
    origin = size = None
    if lo is not None:
        origin = (C.c_int * 3)(*[int(a) for a in lo])
        size = (C.c_int * 3)(*[int(b) - int(a) + 1 for a, b in zip(lo, hi)])
    res = _abi.vrt_redistance_result()
    if lib.vrh_redistance(rec.ctypes.data, vol.N, float(unit), int(bool(texel16)), int(band), int(from_), origin, size, C.byref(res)) != 0:
        raise RuntimeError("vrh_redistance: " + lib.vrh_last_error().decode(errors="replace"))
    vol.density = np.ascontiguousarray(rec["density"].reshape(vol.N, vol.N, vol.N))
    vol.dirty = True
    return {"written": int(res.written), "near": int(res.near), "surfels": int(res.surfels), "lo": tuple(res.lo), "hi": tuple(res.hi)}


def stamp_host(dst: VVoxelVolume, src: VVoxelVolume, stamp: _abi.vrt_stamp, dst_texel16: bool = False, src_texel16: bool = False) -> dict:
    """VVolumeConverter::Stamp (the host build of vrt_volume_stamp's rule) on two volumes' densities and material ids: `src` merged
    into `dst` in place as the record says; each volume's extent and density_scale give its density units.  texel16: that volume's
    densities are the integer field +-q of a TEXEL16 slot.  Raises _abi.VrtError with the code vrt_volume_stamp returns for a record
    it refuses.  Returns {"written", "lo", "hi"} (xyz, inclusive; lo > hi when nothing was written)."""
    lib = load_host()
    dtype = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])
    recs = []
    for vol in (dst, src):
        rec = np.zeros(vol.N ** 3, dtype=dtype)
        rec["density"] = np.asarray(vol.density, np.float32).reshape(-1)
        rec["material"] = np.asarray(vol.material_id, np.uint8).reshape(-1)
        recs.append(rec)
    res = _abi.vrt_brush_result()
    rc = lib.vrh_stamp(recs[0].ctypes.data, dst.N, float(dst.VolumeExtends), float(dst.density_scale), int(bool(dst_texel16)),
                       recs[1].ctypes.data, src.N, float(src.VolumeExtends), float(src.density_scale), int(bool(src_texel16)),
                       C.byref(stamp), C.byref(res))
    _abi.check(rc, "vrh_stamp")
    if res.written:
        dst.density = np.ascontiguousarray(recs[0]["density"].reshape(dst.N, dst.N, dst.N))
        dst.material_id = np.ascontiguousarray(recs[0]["material"].reshape(dst.N, dst.N, dst.N))
        dst.dirty = True
    return {"written": int(res.written), "lo": tuple(res.lo), "hi": tuple(res.hi)}


def smooth_host(vol: VVoxelVolume, smooth: _abi.vrt_smooth, texel16: bool = False) -> dict:
    """VVolumeConverter::Smooth (the host build of vrt_volume_smooth's rule) on a volume's densities and material ids, in place.
    texel16: the densities are the integer field +-q of a TEXEL16 slot.  Raises _abi.VrtError with the code vrt_volume_smooth returns
    for a record it refuses.  Returns {"written", "lo", "hi"} (xyz, inclusive; lo > hi when nothing was written)."""
    lib = load_host()
    dtype = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])
    rec = np.zeros(vol.N ** 3, dtype=dtype)
    rec["density"] = np.asarray(vol.density, np.float32).reshape(-1)
    rec["material"] = np.asarray(vol.material_id, np.uint8).reshape(-1)
    res = _abi.vrt_brush_result()
    rc = lib.vrh_smooth(rec.ctypes.data, vol.N, float(vol.VolumeExtends), float(vol.density_scale), int(bool(texel16)), C.byref(smooth),
                        C.byref(res))
    _abi.check(rc, "vrh_smooth")
    if res.written:
        vol.density = np.ascontiguousarray(rec["density"].reshape(vol.N, vol.N, vol.N))
        vol.material_id = np.ascontiguousarray(rec["material"].reshape(vol.N, vol.N, vol.N))
        vol.dirty = True
    return {"written": int(res.written), "lo": tuple(res.lo), "hi": tuple(res.hi)}


def warp_host(vol: VVoxelVolume, warp: _abi.vrt_warp, texel16: bool = False) -> dict:
    """VVolumeConverter::Warp (the host build of vrt_volume_warp's rule) on a volume's densities and material ids, in place.
    texel16: the densities are the integer field +-q of a TEXEL16 slot.  Raises _abi.VrtError with the code vrt_volume_warp returns
    for a record it refuses.  Returns {"written", "lo", "hi"} (xyz, inclusive; lo > hi when nothing was written)."""
    lib = load_host()
    dtype = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])
    rec = np.zeros(vol.N ** 3, dtype=dtype)
    rec["density"] = np.asarray(vol.density, np.float32).reshape(-1)
    rec["material"] = np.asarray(vol.material_id, np.uint8).reshape(-1)
    res = _abi.vrt_brush_result()
    rc = lib.vrh_warp(rec.ctypes.data, vol.N, float(vol.VolumeExtends), float(vol.density_scale), int(bool(texel16)), C.byref(warp), C.byref(res))
    _abi.check(rc, "vrh_warp")
    if res.written:
        vol.density = np.ascontiguousarray(rec["density"].reshape(vol.N, vol.N, vol.N))
        vol.material_id = np.ascontiguousarray(rec["material"].reshape(vol.N, vol.N, vol.N))
        vol.dirty = True
    return {"written": int(res.written), "lo": tuple(res.lo), "hi": tuple(res.hi)}


def extract_mesh_host(vol: VVoxelVolume, iso: float = 0.0, lo=None, hi=None, texel16: bool = False):
    """VVolumeConverter::ExtractMesh (the host build of vrt_volume_extract_mesh's rule) on a volume's densities and material ids: the
    surface density = iso over the samples lo..hi (inclusive xyz corners; both None: the whole grid) by surface nets.  texel16: the
    densities are the integer field +-q of a TEXEL16 slot.  The volume is only read.  Returns (positions (V, 3) float32 in object space,
    normals (V, 3) float32, materials (V,) uint8, indices (T, 3) uint32, {"vertices", "quads", "lo", "hi"})."""
    lib = load_host()
    if (lo is None) != (hi is None):
        raise ValueError("extract_mesh_host: give both corners of the box or neither")
    rec = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
    rec["density"] = np.asarray(vol.density, np.float32).reshape(-1)
    rec["material"] = np.asarray(vol.material_id, np.uint8).reshape(-1)
    origin = size = None
    if lo is not None:
        origin = (C.c_int * 3)(*[int(a) for a in lo])
        size = (C.c_int * 3)(*[int(b) - int(a) + 1 for a, b in zip(lo, hi)])
    res = _abi.vrt_mesh_result()
    head = (rec.ctypes.data, vol.N, float(vol.VolumeExtends), int(bool(texel16)), float(iso), origin, size)
    if lib.vrh_extract_mesh(*head, None, None, None, 0, None, 0, C.byref(res)) != 0:
        raise RuntimeError("vrh_extract_mesh: " + lib.vrh_last_error().decode(errors="replace"))
    V, Q = int(res.vertices), int(res.quads)
    positions, normals = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
    materials, indices = np.zeros(V, np.uint8), np.zeros((2 * Q, 3), np.uint32)
    if V and lib.vrh_extract_mesh(*head, positions.ctypes.data, normals.ctypes.data, materials.ctypes.data, V, indices.ctypes.data, 6 * Q,
                                  C.byref(res)) != 0:
        raise RuntimeError("vrh_extract_mesh: " + lib.vrh_last_error().decode(errors="replace"))
    return positions, normals, materials, indices, {"vertices": V, "quads": Q, "lo": tuple(res.lo), "hi": tuple(res.hi)}


class vrh_placed_volume(C.Structure):
    """One side of vrh_contacts (csrc/host/host_c_api.cpp)."""
    _fields_ = [("voxels", C.c_void_p), ("n", C.c_int32), ("texel16", C.c_int32), ("extent", C.c_float), ("density_scale", C.c_float),
                ("step_max", C.c_float), ("position", C.c_float * 3), ("rotation", C.c_float * 4), ("scale", C.c_float * 3)]


def contacts_host(stored_a, material_a, placed_a: dict, stored_b, material_b, placed_b: dict, margin: float = 0.0, clip: bool = True) -> dict:
    """VVolumeConverter::Contacts (the host build of vrt_query_contacts' rule): where the surface of volume a touches or enters volume b.
    stored_*: what a slot's dense grid holds, float32 [x, z, y] (texel16: the integer field +-q); material_*: the ids, uint8, same order
    (None: zeros); placed_*: {"extent", and optionally "texel16", "density_scale", "step_max", "position", "rotation" (x, y, z, w),
    "scale"}.  clip = False walks all of a's cells instead of the rule's conservative cell box: the same output.  Returns
    renderer.contacts_to_dict's dict."""
    from .renderer import CONTACT_DTYPE, contacts_to_dict

    lib = load_host()
    keep = []

    def side(stored, material, placed):
        stored = np.asarray(stored, np.float32)
        n = stored.shape[0]
        rec = np.zeros(n ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        rec["density"] = stored.reshape(-1)
        if material is not None:
            rec["material"] = np.asarray(material, np.uint8).reshape(-1)
        keep.append(rec)
        return vrh_placed_volume(rec.ctypes.data, n, int(bool(placed.get("texel16", False))), float(placed["extent"]),
                                 float(placed.get("density_scale", 1.0)), float(placed.get("step_max", 0.0)),
                                 (C.c_float * 3)(*[float(x) for x in placed.get("position", (0.0, 0.0, 0.0))]),
                                 (C.c_float * 4)(*[float(x) for x in placed.get("rotation", (0.0, 0.0, 0.0, 1.0))]),
                                 (C.c_float * 3)(*[float(x) for x in placed.get("scale", (1.0, 1.0, 1.0))]))

    a, b = side(stored_a, material_a, placed_a), side(stored_b, material_b, placed_b)
    res = _abi.vrt_contacts_result()
    if lib.vrh_contacts(C.byref(a), C.byref(b), float(margin), int(bool(clip)), None, 0, C.byref(res)) != 0:
        raise RuntimeError("vrh_contacts: " + lib.vrh_last_error().decode(errors="replace"))
    rec = np.zeros(int(res.contacts), CONTACT_DTYPE)
    if len(rec) and lib.vrh_contacts(C.byref(a), C.byref(b), float(margin), int(bool(clip)), rec.ctypes.data, len(rec), C.byref(res)) != 0:
        raise RuntimeError("vrh_contacts: " + lib.vrh_last_error().decode(errors="replace"))
    return contacts_to_dict(rec, res)


def measure_host(vol: VVoxelVolume, iso: float = 0.0, lo=None, hi=None, texel16: bool = False) -> dict:
    """VVolumeConverter::Measure (the host build of vrt_volume_measure's rule) on a volume's densities and material ids, over the samples
    lo..hi (inclusive xyz corners; both None: the whole grid).  texel16: the densities are the integer field +-q of a TEXEL16 slot.  The
    volume is only read.  Returns _abi.measure_dict's dict: the record's integer fields and "material_samples" (256 counts);
    _abi.mass_properties turns it into volume, area, centroid and inertia."""
    lib = load_host()
    if (lo is None) != (hi is None):
        raise ValueError("measure_host: give both corners of the box or neither")
    rec = np.zeros(vol.N ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
    rec["density"] = np.asarray(vol.density, np.float32).reshape(-1)
    rec["material"] = np.asarray(vol.material_id, np.uint8).reshape(-1)
    origin = size = None
    if lo is not None:
        origin = (C.c_int * 3)(*[int(a) for a in lo])
        size = (C.c_int * 3)(*[int(b) - int(a) + 1 for a, b in zip(lo, hi)])
    res, counts = _abi.vrt_measure_result(), (C.c_uint64 * 256)()
    if lib.vrh_measure(rec.ctypes.data, vol.N, int(bool(texel16)), float(iso), origin, size, C.byref(res), counts) != 0:
        raise RuntimeError("vrh_measure: " + lib.vrh_last_error().decode(errors="replace"))
    return _abi.measure_dict(res, counts)


def import_gltf_mesh(path: str, mesh: int = 0):
    """VGLTFImporter::ImportScene on a .gltf / .glb file: (name, positions (V, 3) float32 as the importer hands them to the converter
    — times 100 and re-centred on the middle of the bounds —, indices uint32) of mesh number `mesh` of the file."""
    lib = load_host()
    counts = (C.c_size_t * 2)()
    name = C.create_string_buffer(256)
    if lib.vrh_gltf_mesh(path.encode(), int(mesh), counts, None, 0, None, 0, name, 256) != 0:
        raise RuntimeError("vrh_gltf_mesh: " + lib.vrh_last_error().decode(errors="replace"))
    positions, indices = np.zeros((counts[0], 3), np.float32), np.zeros(counts[1], np.uint32)
    if lib.vrh_gltf_mesh(path.encode(), int(mesh), counts, positions.ctypes.data, counts[0], indices.ctypes.data, counts[1], name, 256) != 0:
        raise RuntimeError("vrh_gltf_mesh: " + lib.vrh_last_error().decode(errors="replace"))
    return name.value.decode(), positions, indices


def voxelize_file(gltf_path: str, out_path: str | None = None, texlib: str | None = None) -> str:
    lib = load_host()
    buf = C.create_string_buffer(4096)
    rc = lib.vrh_voxelize_file(gltf_path.encode(), texlib.encode() if texlib else None, out_path.encode() if out_path else None, buf, 4096)
    if rc != 0:
        raise RuntimeError("vrh_voxelize_file: " + lib.vrh_last_error().decode(errors="replace"))
    return buf.value.decode()


def vox_rewrite(in_path: str, out_path: str) -> None:
    lib = load_host()
    if lib.vrh_vox_rewrite(in_path.encode(), out_path.encode()) != 0:
        raise RuntimeError("vrh_vox_rewrite: " + lib.vrh_last_error().decode(errors="replace"))


# ---- procedural meshes --------------------------------------------------------------------------

def cube_mesh(half: float = 0.5) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """24 vertices (4 per face, with normals), 12 triangles; positions in glTF units."""
    faces = [((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1), (0, 1, 0)), ((0, 1, 0), (0, 0, 1), (1, 0, 0)),
             ((0, -1, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0), (1, 0, 0))]
    pos, nrm, idx = [], [], []
    for n, u, w in faces:
        n, u, w = np.array(n, float), np.array(u, float), np.array(w, float)
        base = len(pos)
        for su, sw in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            pos.append((n + su * u + sw * w) * half)
            nrm.append(n)
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.array(pos, np.float32), np.array(nrm, np.float32), np.array(idx, np.uint32)


def torus_mesh(major: float = 0.55, minor: float = 0.22, nu: int = 128, nv: int = 64) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """UV torus around the Z axis (seedless), positions in glTF units."""
    u = np.arange(nu) * (2 * math.pi / nu)
    v = np.arange(nv) * (2 * math.pi / nv)
    U, V = np.meshgrid(u, v, indexing="ij")
    x = (major + minor * np.cos(V)) * np.cos(U)
    y = (major + minor * np.cos(V)) * np.sin(U)
    z = minor * np.sin(V)
    pos = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    nrm = np.stack([np.cos(V) * np.cos(U), np.cos(V) * np.sin(U), np.sin(V)], -1).reshape(-1, 3).astype(np.float32)
    idx = []
    for i in range(nu):
        for j in range(nv):
            a = i * nv + j
            b = ((i + 1) % nu) * nv + j
            c = ((i + 1) % nu) * nv + (j + 1) % nv
            d = i * nv + (j + 1) % nv
            idx += [a, b, c, a, c, d]
    return pos, nrm, np.array(idx, np.uint32)


def importer_space(positions: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """What VGLTFImporter does to POSITION data (GLTFImporter.cpp:52-64,111-121): scale by 100,
    re-centre on the accessor's min/max midpoint; bounds extents = half size + 5."""
    p = positions.astype(np.float32)
    mn = p.min(0) * np.float32(100.0)
    mx = p.max(0) * np.float32(100.0)
    ext = (mx - mn) * np.float32(0.5)
    off = mx - ext
    return p * np.float32(100.0) - off, ext + np.float32(5.0)


def write_gltf(path: str, meshes, nodes, materials=None, embed: bool = False) -> None:
    """Minimal .gltf (+ .bin) writer.  meshes: list of (name, positions, normals, indices, material
    index or None); nodes: list of dicts (name, mesh, translation, rotation, scale, extras)."""
    blob = bytearray()
    views, accessors, gm = [], [], []

    def add(data: np.ndarray, target: int, comp: int, typ: str, minmax: bool):
        while len(blob) % 4:
            blob.append(0)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": data.nbytes, "target": target})
        blob.extend(data.tobytes())
        acc = {"bufferView": len(views) - 1, "componentType": comp, "count": int(data.shape[0]), "type": typ}
        if minmax:
            acc["min"] = [float(x) for x in data.min(0)]
            acc["max"] = [float(x) for x in data.max(0)]
        accessors.append(acc)
        return len(accessors) - 1

    for name, pos, nrm, idx, mat in meshes:
        use16 = len(pos) < 65536
        ia = add(idx.astype(np.uint16 if use16 else np.uint32).reshape(-1), 34963, 5123 if use16 else 5125, "SCALAR", False)
        pa = add(pos.astype(np.float32), 34962, 5126, "VEC3", True)
        na = add(nrm.astype(np.float32), 34962, 5126, "VEC3", False)
        prim = {"attributes": {"POSITION": pa, "NORMAL": na}, "indices": ia}
        if mat is not None:
            prim["material"] = mat
        gm.append({"name": name, "primitives": [prim]})
    bin_name = os.path.splitext(os.path.basename(path))[0] + ".bin"
    buf = {"byteLength": len(blob)}
    buf["uri"] = ("data:application/octet-stream;base64," + base64.b64encode(bytes(blob)).decode()) if embed else bin_name
    doc = {"asset": {"version": "2.0", "generator": "volumetricraytracer_amd tests"}, "buffers": [buf], "bufferViews": views,
           "accessors": accessors, "meshes": gm, "nodes": nodes, "scenes": [{"nodes": list(range(len(nodes)))}], "scene": 0}
    if materials:
        doc["materials"] = materials
    with open(path, "w") as f:
        json.dump(doc, f)
    if not embed:
        with open(os.path.join(os.path.dirname(path), bin_name), "wb") as f:
            f.write(bytes(blob))


def gltf_to_glb(gltf_path: str, glb_path: str) -> None:
    """Packs a .gltf with ONE external .bin buffer into a binary .glb container (glTF 2.0 spec §4.4)."""
    import json
    import struct

    doc = json.load(open(gltf_path))
    if len(doc.get("buffers", [])) != 1 or doc["buffers"][0].get("uri", "").startswith("data:"):
        raise ValueError("expects exactly one external buffer")
    blob = open(os.path.join(os.path.dirname(gltf_path), doc["buffers"][0].pop("uri")), "rb").read()
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    blob += b"\0" * (-len(blob) % 4)
    total = 12 + 8 + len(js) + 8 + len(blob)
    with open(glb_path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, total))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        f.write(struct.pack("<II", len(blob), 0x004E4942) + blob)


def load_texture(path: str) -> np.ndarray:
    """Decodes a material texture file (PNG or binary PPM) with the C++ host loader VHipRenderer uses for
    VMaterial texture paths; returns uint8 [H, W, 4]."""
    lib = load_host()
    lib.vrh_texture_load.restype = C.c_int
    lib.vrh_texture_load.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]
    w, h = C.c_int(), C.c_int()
    if lib.vrh_texture_load(path.encode(), C.byref(w), C.byref(h), None, 0) != 0:
        raise RuntimeError("vrh_texture_load: " + lib.vrh_last_error().decode(errors="replace"))
    out = np.zeros((h.value, w.value, 4), np.uint8)
    if lib.vrh_texture_load(path.encode(), None, None, out.ctypes.data, out.nbytes) != 0:
        raise RuntimeError("vrh_texture_load: " + lib.vrh_last_error().decode(errors="replace"))
    return out


def load_skybox_faces(directory: str) -> np.ndarray:
    """Sky box from <directory>/XP.png ... ZM.png (the reference's Resources/Skybox layout), or from a .dds cube map (what
    VTextureFactory::LoadTextureCubeFromFile reads: uncompressed RGBA / BGRA / BGRX / RGB, top mip), through the C++ host
    loader; returns uint8 [6, S, S, 4] in the order vrt_env_upload / VScene.EnvironmentMap expect (+X,-X,+Y,-Y,+Z,-Z)."""
    lib = load_host()
    lib.vrh_cubemap_load.restype = C.c_int
    lib.vrh_cubemap_load.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_void_p, C.c_size_t]
    size = C.c_int()
    if lib.vrh_cubemap_load(directory.encode(), C.byref(size), None, 0) != 0:
        raise RuntimeError("vrh_cubemap_load: " + lib.vrh_last_error().decode(errors="replace"))
    out = np.zeros((6, size.value, size.value, 4), np.uint8)
    if lib.vrh_cubemap_load(directory.encode(), None, out.ctypes.data, out.nbytes) != 0:
        raise RuntimeError("vrh_cubemap_load: " + lib.vrh_last_error().decode(errors="replace"))
    return out
