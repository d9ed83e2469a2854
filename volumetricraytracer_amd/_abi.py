"""ctypes mirror of include/vrt.h and the loader of the in-tree C-ABI library.

The library (volumetricraytracer_amd/lib/libvrt_hip.so) is the product; this module only
declares its entry points.  There is no fallback: if the library is missing or fails to load,
`load()` raises — nothing here can render on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os

VRT_MAX_VOLUMES = 20
VRT_MAX_TEXTURES = 64
VRT_FRAMES_IN_FLIGHT = 3
VRT_MAX_RESOLUTION = 9
VRT_MAX_POINT_LIGHTS = 5
VRT_MAX_SPOT_LIGHTS = 5
VRT_MAX_INSTANCES = 64
VRT_MAX_DEVICES = 8
VRT_COMM_ID_BYTES = 128

VRT_OK = 0
VRT_ERR_INVALID = -1
VRT_ERR_NO_DEVICE = -2
VRT_ERR_HIP = -3
VRT_ERR_OOM = -4
VRT_ERR_SLOT = -5
VRT_ERR_NOT_READY = -6
VRT_ERR_UNSUPPORTED = -7

# EVRenderMode (reference Renderer/Public/Renderer.h:32-42)
MODE_INTERP = 0
MODE_INTERP_UNLIT = 1
MODE_INTERP_NOTEX = 2
MODE_INTERP_NOTEX_UNLIT = 3
MODE_CUBE = 4
MODE_CUBE_UNLIT = 5
MODE_CUBE_NOTEX = 6
MODE_CUBE_NOTEX_UNLIT = 7

FORM_FULL, FORM_PASSES, FORM_TEXTURED, FORM_MAY_BOUNCE, FORM_LEAN_REF, FORM_PALETTE = 1, 2, 4, 8, 16, 32  # vrt_debug_last_kernel_form
VRT_MAX_PALETTE = 256
FLAG_DIAG_TIMELINE = 4
FLAG_OUTPUT_RGBA8 = 8
FLAG_NO_TIMING = 16
FLAG_BLOCK_PER_FRAME = 64
FLAG_NO_CULL_RECT = 128
FLAG_FULL_ONE_KERNEL = 256   # full closest hit of a block of frames as ONE kernel (default: three passes)
FLAG_FULL_THREE_PASS = 512   # ... and three passes even for a lone frame
FLAG_OUTPUT_BGRA8 = 2048       # with FLAG_OUTPUT_RGBA8: B8G8R8A8 byte order, the reference's back buffer (DXConstants.cpp:21)
FLAG_REFERENCE_VIEW_VECTOR = 4096      # shade the camera ray's hit with the reference's un-normalised wo, back its secondary rays off 0.1 |dir|
FLAG_REFERENCE_BOUNDARY_TEXELS = 8192  # normal taps beyond the grid read texel 0 (the reference's out-of-bounds Load) instead of the clamped cell
FLAG_NO_HIT_POLISH = 1024     # closest hits stay at the cone threshold's stop point (rounds 1-3) instead of moving on to the crossing
HIT_POLISH_SAMPLES = 2
MAX_BLOCK_FRAMES = 48  # frames one march launch covers with their cameras in the kernarg segment (csrc/vrt_device.h kMaxBlockFrames)
MAX_LAUNCH_FRAMES = 256  # ... with their cameras copied to device memory ahead of the launch: vrt_block.n_frames' upper bound

# vrt_debug_volume_bytes: which device buffer of a slot
VOLUME_BYTES_DENSE, VOLUME_BYTES_MATERIAL, VOLUME_BYTES_BRICKS, VOLUME_BYTES_CELLS = 0, 1, 2, 3
VOLUME_BYTES_SKIP, VOLUME_BYTES_NIB, VOLUME_BYTES_CUBE_SKIP, VOLUME_BYTES_ACTIVE_BOX = 4, 5, 6, 7

FORMAT_F32 = 0
FORMAT_TEXEL16 = 1

PATH_AUTO = 0
PATH_DENSE = 1
PATH_BRICK = 2
PATH_BRICK_LDS = 3
PATH_CELLS = 4

# vrt_volume_apply_brushes
MAX_BRUSHES = 32
BRUSH_SPHERE, BRUSH_BOX, BRUSH_CAPSULE = 0, 1, 2
BRUSH_ADD, BRUSH_SUBTRACT, BRUSH_PAINT = 0, 1, 2

# vrt_volume_stamp
STAMP_ADD, STAMP_SUBTRACT, STAMP_REPLACE = 0, 1, 2
STAMP_MATERIAL_KEEP, STAMP_MATERIAL_SOURCE = -1, -2

# vrt_volume_smooth
MAX_SMOOTH_ITERATIONS = 16
# vrt_volume_warp
WARP_MATERIAL_KEEP, WARP_MATERIAL_SOURCE = -1, -2

# vrt_volume_components
COMPONENTS_REPORT, COMPONENTS_KEEP_LARGEST, COMPONENTS_REMOVE_SMALL, COMPONENTS_KEEP_SEED, COMPONENTS_REMOVE_SEED = 0, 1, 2, 3, 4

QUERY_CLOSEST = 0
QUERY_ANY = 1  # occlusion: instance 0 when some surface lies within [0, t_max]


class vrt_voxel(C.Structure):
    _fields_ = [("material", C.c_uint8), ("pad_", C.c_uint8 * 3), ("density", C.c_float)]


class vrt_material(C.Structure):
    _fields_ = [("tint", C.c_float * 4), ("roughness", C.c_float), ("metallic", C.c_float)]


class vrt_instance(C.Structure):
    _fields_ = [
        ("volume_slot", C.c_int32),
        ("position", C.c_float * 3),
        ("rotation", C.c_float * 4),
        ("scale", C.c_float * 3),
    ]


class vrt_point_light(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("color", C.c_float * 3),
        ("intensity", C.c_float),
        ("att_linear", C.c_float),
        ("att_exp", C.c_float),
    ]


class vrt_spot_light(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("forward", C.c_float * 3),
        ("color", C.c_float * 3),
        ("intensity", C.c_float),
        ("att_linear", C.c_float),
        ("att_exp", C.c_float),
        ("cos_angle", C.c_float),
        ("cos_falloff_angle", C.c_float),
    ]


class vrt_scene(C.Structure):
    _fields_ = [
        ("cam_position", C.c_float * 3),
        ("cam_rotation", C.c_float * 4),
        ("cam_fov_deg", C.c_float),
        ("cam_near", C.c_float),
        ("cam_far", C.c_float),
        ("light_dir", C.c_float * 3),
        ("light_strength", C.c_float),
        ("n_instances", C.c_int32),
        ("n_point_lights", C.c_int32),
        ("n_spot_lights", C.c_int32),
        ("pad_", C.c_int32),
        ("instances", vrt_instance * VRT_MAX_INSTANCES),
        ("point_lights", vrt_point_light * VRT_MAX_POINT_LIGHTS),
        ("spot_lights", vrt_spot_light * VRT_MAX_SPOT_LIGHTS),
    ]


class vrt_params(C.Structure):
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("max_steps", C.c_int32),
        ("shadow", C.c_int32),
        ("mode", C.c_int32),
        ("path", C.c_int32),
        ("max_bounces", C.c_int32),
        ("flags", C.c_int32),
        ("eps_hit", C.c_float),
        ("eps_in", C.c_float),
        ("step_min", C.c_float),
        ("k_relax", C.c_float),
        ("cone_eps", C.c_float),
    ]


class vrt_timing(C.Structure):
    _fields_ = [
        ("kernel_ms", C.c_float),
        ("gather_ms", C.c_float),
        ("total_ms", C.c_float),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("primary_rays", C.c_uint64),
        ("shadow_rays", C.c_uint64),
        ("bounce_rays", C.c_uint64),
        ("primary_steps", C.c_uint64),
        ("shadow_steps", C.c_uint64),
        ("hits", C.c_uint64),
        ("exhausted_rays", C.c_uint64),
    ]


# name -> (restype, argtypes); every symbol include/vrt.h declares
class vrt_camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("rotation", C.c_float * 4), ("fov_deg", C.c_float)]


class vrt_block(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int32),
        ("strip_rows", C.c_int32),
        ("first_strip", C.c_int32),
        ("strip_stride", C.c_int32),
        ("n_strips", C.c_int32),
        ("row0", C.c_int32),
        ("rows", C.c_int32),
        ("cameras", C.POINTER(vrt_camera)),
        ("frame_stride_bytes", C.c_uint64),
        ("scenes", C.POINTER(vrt_scene)),
    ]


class vrt_ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("direction", C.c_float * 3), ("reserved_", C.c_float)]


class vrt_hit(C.Structure):
    _fields_ = [
        ("t", C.c_float),
        ("normal", C.c_float * 3),
        ("instance", C.c_int32),
        ("voxel", C.c_int32 * 3),
        ("material", C.c_uint32),
        ("steps", C.c_uint32),
        ("reserved_", C.c_uint32 * 2),
    ]


MAX_PROJECT_ITERATIONS = 16
POINT_SAMPLED = 1  # vrt_point_result.flags bit 0


class vrt_point(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("reserved_", C.c_float)]


class vrt_point_result(C.Structure):
    _fields_ = [
        ("distance", C.c_float),
        ("normal", C.c_float * 3),
        ("instance", C.c_int32),
        ("voxel", C.c_int32 * 3),
        ("material", C.c_uint32),
        ("flags", C.c_uint32),
        ("moves", C.c_uint32),
        ("position", C.c_float * 3),
        ("reserved_", C.c_uint32 * 2),
    ]


MAX_SWEEP_STEPS = 4096
SWEEP_HIT, SWEEP_EXHAUSTED, SWEEP_INITIAL = 1, 2, 4  # vrt_sweep_hit.flags


class vrt_sweep(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("direction", C.c_float * 3), ("radius", C.c_float)]


class vrt_sweep_hit(C.Structure):
    _fields_ = [
        ("t", C.c_float),
        ("normal", C.c_float * 3),
        ("instance", C.c_int32),
        ("voxel", C.c_int32 * 3),
        ("material", C.c_uint32),
        ("flags", C.c_uint32),
        ("steps", C.c_uint32),
        ("distance", C.c_float),
        ("position", C.c_float * 3),
        ("reserved_", C.c_uint32),
    ]


class vrt_contact(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("distance", C.c_float),
        ("normal", C.c_float * 3),
        ("material_a", C.c_uint32),
        ("normal_a", C.c_float * 3),
        ("material_b", C.c_uint32),
        ("cell_a", C.c_int32 * 3),
        ("reserved_", C.c_uint32),
    ]


class vrt_contacts_result(C.Structure):
    _fields_ = [
        ("lo", C.c_int32 * 3),
        ("hi", C.c_int32 * 3),
        ("contacts", C.c_uint64),
        ("candidates", C.c_uint64),
        ("min_distance", C.c_float),
        ("reserved_", C.c_uint32),
    ]


def contacts_result_dict(res: "vrt_contacts_result") -> dict:
    """A vrt_contacts_result as plain Python values."""
    return {"lo": tuple(res.lo), "hi": tuple(res.hi), "contacts": int(res.contacts), "candidates": int(res.candidates),
            "min_distance": float(res.min_distance)}


class vrt_brush(C.Structure):
    _fields_ = [
        ("shape", C.c_int32),
        ("op", C.c_int32),
        ("a", C.c_float * 3),
        ("b", C.c_float * 3),
        ("radius", C.c_float),
        ("blend", C.c_float),
        ("reach", C.c_float),
        ("material", C.c_int32),
        ("reserved_", C.c_uint32 * 4),
    ]


class vrt_brush_result(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("written", C.c_uint64)]


class vrt_stamp(C.Structure):
    _fields_ = [
        ("op", C.c_int32),
        ("material", C.c_int32),
        ("dst_to_src", C.c_float * 12),
        ("length_scale", C.c_float),
        ("offset", C.c_float),
        ("blend", C.c_float),
        ("reach", C.c_float),
        ("reserved_", C.c_uint32 * 6),
    ]


class vrt_smooth(C.Structure):
    _fields_ = [
        ("shape", C.c_int32),
        ("iterations", C.c_int32),
        ("a", C.c_float * 3),
        ("b", C.c_float * 3),
        ("radius", C.c_float),
        ("strength", C.c_float),
        ("falloff", C.c_float),
        ("rebound", C.c_float),
        ("material", C.c_int32),
        ("reserved_", C.c_uint32 * 3),
    ]


class vrt_warp(C.Structure):
    _fields_ = [
        ("shape", C.c_int32),
        ("material", C.c_int32),
        ("a", C.c_float * 3),
        ("b", C.c_float * 3),
        ("radius", C.c_float),
        ("strength", C.c_float),
        ("falloff", C.c_float),
        ("pull", C.c_float * 12),
        ("length_scale", C.c_float),
        ("inflate", C.c_float),
        ("reserved_", C.c_uint32 * 7),
    ]


class vrt_components(C.Structure):
    _fields_ = [
        ("op", C.c_int32),
        ("material", C.c_int32),
        ("seed", C.c_int32 * 3),
        ("gap", C.c_float),
        ("min_samples", C.c_uint64),
        ("reserved_", C.c_uint32 * 8),
    ]


class vrt_component(C.Structure):
    _fields_ = [("first", C.c_int32 * 3), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("removed", C.c_uint32), ("samples", C.c_uint64)]


class vrt_components_result(C.Structure):
    _fields_ = [
        ("lo", C.c_int32 * 3),
        ("hi", C.c_int32 * 3),
        ("written", C.c_uint64),
        ("solid", C.c_uint64),
        ("removed_samples", C.c_uint64),
        ("components", C.c_uint32),
        ("removed", C.c_uint32),
        ("listed", C.c_uint32),
        ("reserved_", C.c_uint32),
    ]


def components_record(op: int, gap: float = 0.0, material: int = -1, min_samples: int = 0, seed=(0, 0, 0)) -> "vrt_components":
    """A vrt_components record (vrt.h): op COMPONENTS_*; gap in density units; seed xyz for the seed ops."""
    r = vrt_components()
    r.op, r.material, r.gap, r.min_samples = int(op), int(material), float(gap), int(min_samples)
    for i in range(3):
        r.seed[i] = int(seed[i])
    return r


def components_dict(res: "vrt_components_result", listed) -> dict:
    """What vrt_volume_components reported, as plain Python: the result's fields, and "list": one dict per record written."""
    out = {"lo": tuple(res.lo), "hi": tuple(res.hi), "written": int(res.written), "solid": int(res.solid),
           "removed_samples": int(res.removed_samples), "components": int(res.components), "removed": int(res.removed)}
    out["list"] = [{"first": tuple(c.first), "lo": tuple(c.lo), "hi": tuple(c.hi), "removed": int(c.removed), "samples": int(c.samples)}
                   for c in listed[:res.listed]]
    return out


class vrt_fill_result(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("filled", C.c_uint64), ("sweeps", C.c_uint32), ("reserved_", C.c_uint32)]


class vrt_redistance_result(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("written", C.c_uint64), ("near", C.c_uint64), ("surfels", C.c_uint32),
                ("reserved_", C.c_uint32)]


class vrt_mesh_result(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("vertices", C.c_uint64), ("quads", C.c_uint64)]


class vrt_measure_result(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("subsamples", C.c_uint64), ("moment1", C.c_uint64 * 3),
                ("moment2", C.c_uint64 * 6), ("solid_samples", C.c_uint64), ("active_cells", C.c_uint64), ("crossings", C.c_uint64 * 3),
                ("quads", C.c_uint64), ("area_q", C.c_uint64), ("reserved_", C.c_uint64 * 2)]


class vrt_mass_properties(C.Structure):
    _fields_ = [("volume", C.c_double), ("area", C.c_double), ("centroid", C.c_double * 3), ("inertia", C.c_double * 6),
                ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3)]


MEASURE_SUBSAMPLES = 4


def measure_dict(res: "vrt_measure_result", counts=None) -> dict:
    """A vrt_measure_result (and the 256 material counts) as plain Python ints."""
    out = {"lo": tuple(res.lo), "hi": tuple(res.hi), "subsamples": int(res.subsamples), "moment1": tuple(int(x) for x in res.moment1),
           "moment2": tuple(int(x) for x in res.moment2), "solid_samples": int(res.solid_samples), "active_cells": int(res.active_cells),
           "crossings": tuple(int(x) for x in res.crossings), "quads": int(res.quads), "area_q": int(res.area_q)}
    if counts is not None:
        out["material_samples"] = tuple(int(x) for x in counts)
    return out


def measure_record(m: dict) -> "vrt_measure_result":
    """The way back from measure_dict."""
    res = vrt_measure_result()
    res.lo[:], res.hi[:] = m["lo"], m["hi"]
    res.moment1[:], res.moment2[:], res.crossings[:] = m["moment1"], m["moment2"], m["crossings"]
    for name in ("subsamples", "solid_samples", "active_cells", "quads", "area_q"):
        setattr(res, name, m[name])
    return res


def mass_properties(m: dict, resolution: int, extent: float) -> dict:
    """vrt_measure_properties (host only) on a measure_dict: {"volume", "area", "centroid", "inertia", "box_lo", "box_hi"} as floats, in
    the volume's object space, for unit density."""
    out = vrt_mass_properties()
    check(load().vrt_measure_properties(C.byref(measure_record(m)), int(resolution), float(extent), C.byref(out)), "vrt_measure_properties")
    return {"volume": out.volume, "area": out.area, "centroid": tuple(out.centroid), "inertia": tuple(out.inertia),
            "box_lo": tuple(out.box_lo), "box_hi": tuple(out.box_hi)}


class vrt_history_info(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("max_entries", C.c_int32), ("max_bytes", C.c_uint64), ("undo_entries", C.c_uint32),
                ("redo_entries", C.c_uint32), ("bytes", C.c_uint64), ("dropped", C.c_uint64), ("top_tiles", C.c_uint64),
                ("reserved_", C.c_uint32 * 4)]


# vrt_volume_history: a history tile is 4^3 samples and costs HISTORY_TILE_BYTES of device memory
HISTORY_TILE = 4
HISTORY_TILE_BYTES = 336

REDISTANCE_FROM_BOTH, REDISTANCE_FROM_OUTSIDE, REDISTANCE_FROM_INSIDE = 0, 1, 2

# vrt_volume_mask_apply
MAX_MASK_OPS = 32
MAX_MASK_STEPS = 64
MASK_ALL, MASK_SHAPE, MASK_MATERIAL, MASK_SOLID, MASK_INVERT, MASK_GROW, MASK_SHRINK = 0, 1, 2, 3, 4, 5, 6


class vrt_mask_op(C.Structure):
    _fields_ = [("kind", C.c_int32), ("value", C.c_int32), ("shape", C.c_int32), ("a", C.c_float * 3), ("b", C.c_float * 3),
                ("radius", C.c_float), ("material", C.c_int32), ("steps", C.c_int32), ("reserved_", C.c_uint32 * 4)]


class vrt_mask_info(C.Structure):
    _fields_ = [("on", C.c_int32), ("pad_", C.c_int32), ("masked", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
                ("restored", C.c_uint64)]


def mask_op(kind: int, value: int = 0, shape: int = 0, a=(0.0, 0.0, 0.0), b=(0.0, 0.0, 0.0), radius: float = 0.0, material: int = 0,
            steps: int = 0) -> "vrt_mask_op":
    """A vrt_mask_op record (vrt.h): kind MASK_*; value 1 protects and 0 releases; shape, a, b, radius as a vrt_brush has them."""
    r = vrt_mask_op()
    r.kind, r.value, r.shape, r.radius, r.material, r.steps = int(kind), int(value), int(shape), float(radius), int(material), int(steps)
    for i in range(3):
        r.a[i], r.b[i] = float(a[i]), float(b[i])
    return r


def mask_info_dict(info: "vrt_mask_info") -> dict:
    """A vrt_mask_info as plain Python values."""
    return {"on": int(info.on), "masked": int(info.masked), "lo": tuple(info.lo), "hi": tuple(info.hi), "restored": int(info.restored)}

SYMBOLS = {
    "vrt_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]),
    "vrt_destroy": (C.c_int, [C.c_void_p]),
    "vrt_volume_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_uint8, C.c_float, C.c_void_p, C.c_void_p]),
    "vrt_volume_upload_voxels": (C.c_int, [C.c_void_p, C.c_int, C.c_uint8, C.c_float, C.c_void_p]),
    "vrt_set_volume_format": (C.c_int, [C.c_void_p, C.c_int]),
    "vrt_volume_upload_texels": (C.c_int, [C.c_void_p, C.c_int, C.c_uint8, C.c_float, C.c_void_p]),
    "vrt_volume_set_material": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(vrt_material)]),
    "vrt_volume_set_palette": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(vrt_material)]),
    "vrt_volume_get_palette": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(vrt_material), C.POINTER(C.c_int)]),
    "vrt_volume_set_metric": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "vrt_texture_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vrt_texture_free": (C.c_int, [C.c_void_p, C.c_int]),
    "vrt_volume_set_textures": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]),
    "vrt_voxelize_mesh": (C.c_int, [C.c_void_p, C.c_int, C.c_uint8, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    "vrt_volume_download": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vrt_volume_free": (C.c_int, [C.c_void_p, C.c_int]),
    "vrt_volume_update_region": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    "vrt_volume_update_voxels": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "vrt_volume_apply_brushes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(vrt_brush), C.POINTER(vrt_brush_result)]),
    "vrt_volume_stamp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(vrt_stamp), C.POINTER(vrt_brush_result)]),
    "vrt_volume_smooth": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(vrt_smooth), C.POINTER(vrt_brush_result)]),
    "vrt_volume_warp": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(vrt_warp), C.POINTER(vrt_brush_result)]),
    "vrt_volume_components": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(vrt_components), C.POINTER(vrt_component), C.c_int,
                                        C.POINTER(vrt_components_result)]),
    "vrt_volume_fill_enclosed": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.POINTER(vrt_fill_result)]),
    "vrt_volume_redistance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(vrt_redistance_result)]),
    "vrt_volume_extract_mesh": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(vrt_mesh_result)]),
    "vrt_volume_measure": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(vrt_measure_result),
                                     C.POINTER(C.c_uint64)]),
    "vrt_measure_properties": (C.c_int, [C.POINTER(vrt_measure_result), C.c_uint8, C.c_float, C.POINTER(vrt_mass_properties)]),
    "vrt_volume_download_region": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "vrt_volume_history": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint64]),
    "vrt_volume_history_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(vrt_history_info)]),
    "vrt_volume_undo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(vrt_brush_result)]),
    "vrt_volume_redo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(vrt_brush_result)]),
    "vrt_volume_mask_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(vrt_mask_op), C.POINTER(vrt_mask_info)]),
    "vrt_volume_mask_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vrt_volume_mask_download": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vrt_volume_mask_clear": (C.c_int, [C.c_void_p, C.c_int]),
    "vrt_volume_mask_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(vrt_mask_info)]),
    "vrt_debug_volume_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vrt_env_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vrt_scene_set": (C.c_int, [C.c_void_p, C.POINTER(vrt_scene)]),
    "vrt_render": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.c_void_p]),
    "vrt_render_rows": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vrt_render_strips": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vrt_render_block": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.POINTER(vrt_block), C.c_void_p, C.c_void_p]),
    "vrt_render_block_host": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.POINTER(vrt_block), C.POINTER(C.c_void_p)]),
    "vrt_comm_unique_id": (C.c_int, [C.c_void_p]),
    "vrt_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vrt_comm_destroy": (C.c_int, [C.c_void_p]),
    "vrt_comm_expect_sizes": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t]),
    "vrt_gather_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "vrt_exchange_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "vrt_render_begin": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.c_int]),
    "vrt_render_end": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "vrt_trace_rays": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_trace_rays_host": (C.c_int, [C.c_void_p, C.POINTER(vrt_params), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vrt_camera_rays": (C.c_int, [C.POINTER(vrt_scene), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vrt_query_points": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_query_points_host": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "vrt_query_sweeps": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_query_sweeps_host": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "vrt_query_contacts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_size_t, C.POINTER(vrt_contacts_result)]),
    "vrt_last_timing": (C.c_int, [C.c_void_p, C.POINTER(vrt_timing)]),
    "vrt_timing_history": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "vrt_launch_history": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "vrt_debug_wave_records": (C.c_longlong, [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]),
    "vrt_debug_last_kernel_form": (C.c_int, [C.c_void_p]),
    "vrt_debug_gather_ceiling": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_float)]),
    "vrt_strerror": (C.c_char_p, [C.c_int]),
    "vrt_version": (C.c_char_p, []),
}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libvrt_hip.so")

_lib = None


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so.7 /
    libhsa-runtime64; if ours (from /opt/rocm) is loaded first and torch's second, the second
    ROCr instance finds no GPU.  Both have the soname libamdhip64.so.7, so importing torch
    first makes the dynamic loader resolve our DT_NEEDED entry to the copy torch already
    mapped.  Without torch installed this is a no-op and the system ROCm runtime is used."""
    import sys

    if "torch" in sys.modules or os.environ.get("VRT_NO_TORCH_PRELOAD") == "1":
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load(path: str | None = None) -> C.CDLL:
    """Load libvrt_hip.so and bind every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("VRT_LIB") or LIB_PATH  # VRT_LIB: an A/B build of the same library (tools/ab_lib_variants.sh)
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} is missing: the HIP library is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or volumetricraytracer_amd/csrc/build.sh). "
            "There is no CPU fallback."
        )
    _share_hip_runtime_with_torch()
    lib = C.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


class VrtError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        try:
            msg = load().vrt_strerror(status).decode()
        except Exception:  # pragma: no cover - only if the library vanished
            msg = "?"
        super().__init__(f"{what}: {msg} ({status})")


def check(status: int, what: str) -> None:
    if status != VRT_OK:
        raise VrtError(status, what)
