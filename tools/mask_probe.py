"""GPU probe (not part of the suite): what a slot mask (vrt_volume_mask_*) costs an edit call, and that a slot without one pays nothing,
on workloads.voxelized_torus(8), the benched 256^3 voxelized-mesh volume (257^3 samples), in both device formats.  The calls: one hard
SUBTRACT sphere dab of 16 cells on the solid's surface, one smooth of the same ball (strength 0.5, two iterations), the fill of the
shell, and a whole-grid redistance (band 3, FROM_OUTSIDE).  Variants, taking turns call by call:
  parent     the call through the parent commit's library (--parent LIB, built beside this one with VRT_LIB_NAME), which has no masks;
  none       through this library, no mask on the slot: must cost what `parent` costs;
  half       the half x < N / 2 protected: one footprint copy and one put-back pass, both clipped to the box of the set bits;
  unclipped  the same half plus the one sample (N-1, N-1, N-1), so that the set bits' box is the whole grid and the clip gains nothing.
Every timed call follows an untimed upload of the same field (and the mask records), so every call meets the same samples.  Times are
host wall times around calls that end in a synchronise.  The first round is not counted; a block is the median of --reps rounds, and
the spread of the --blocks block medians (max - min) is the run-to-run noise.  Prints one JSON line.

    python tools/mask_probe.py --parent volumetricraytracer_amd/lib/libvrt_hip_parent.so [--reps 3] [--blocks 3] [--formats f32,texel16]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import volumetricraytracer_amd as v  # noqa: E402
from volumetricraytracer_amd import _abi  # noqa: E402
from volumetricraytracer_amd import workloads  # noqa: E402

RADIUS = 16.0
CALLS = ("dab", "smooth", "fill", "redistance")
VARIANTS = ("parent", "none", "half", "unclipped")


def load_parent(path):
    """The parent's library with the entry points it has (it lacks the masks')."""
    lib = C.CDLL(path)
    for name, (res, args) in _abi.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def renderer(lib):
    r = v.VHipRenderer()
    if lib is not None:
        r._lib = lib
    assert r.Start()
    return r


def mask_records(N, variant):
    c = (N - 1) / 2.0
    ops = [_abi.mask_op(_abi.MASK_SHAPE, 1, _abi.BRUSH_BOX, a=(0.0, c, c), b=(N // 2 - 0.5, float(N), float(N)))]
    if variant == "unclipped":
        ops.append(_abi.mask_op(_abi.MASK_SHAPE, 1, _abi.BRUSH_SPHERE, a=(N - 1.0, N - 1.0, N - 1.0), radius=0.25))
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's library, built with VRT_LIB_NAME beside this one")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--formats", default="f32,texel16")
    args = ap.parse_args()
    out = {"reps": args.reps, "blocks": args.blocks, "unit": "ms, median wall time around the call, one value per block", "dab_radius_cells": RADIUS}
    shell = workloads.voxelized_torus(8)
    N = shell.N
    for name in args.formats.split(","):
        fmt = _abi.FORMAT_TEXEL16 if name == "texel16" else _abi.FORMAT_F32
        vol = shell.set_device_format(fmt)
        ctx = {k: renderer(load_parent(args.parent) if k == "parent" else None) for k in VARIANTS}
        # the filled solid, for the calls that edit one: what the fill leaves, as this library's context downloads it
        ctx["none"].upload_volume(0, vol)
        ctx["none"].fill_enclosed(0, None, 1.0, 1)
        solid = ctx["none"].download_volume(0, vol.Resolution, vol.VolumeExtends).set_device_format(fmt)
        solid.density_scale, solid.step_max = vol.density_scale, vol.step_max
        inside = np.argwhere(np.asarray(solid.density) <= 0)
        x, z, y = inside[len(inside) // 2]  # a sample of the solid on the plane the mask ends at, or near it
        at = (float(N // 2), float(y), float(z)) if solid.density[N // 2, z, y] <= 0 else (float(x), float(y), float(z))
        brush = [v.sphere_brush(_abi.BRUSH_SUBTRACT, at, RADIUS, 0.0, 2.0, 0)]
        smooth = v.smooth_record(shape=_abi.BRUSH_SPHERE, a=at, b=(0.0, 0.0, 0.0), radius=RADIUS, strength=0.5, iterations=2, falloff=0.5 * RADIUS,
                                 rebound=0.0, material=-1)
        run = {"dab": lambda r: r.apply_brushes(0, None, brush), "smooth": lambda r: r.smooth_volume(0, smooth),
               "fill": lambda r: r.fill_enclosed(0, None, 1.0, 1), "redistance": lambda r: r.redistance(0, None, 3, _abi.REDISTANCE_FROM_OUTSIDE)}
        got, info, turn = {}, {}, 0

        def one(call, variant):
            r = ctx[variant]
            r.upload_volume(0, vol if call == "fill" else solid)  # untimed; drops the mask
            if variant in ("half", "unclipped"):
                info[variant] = r.mask_apply(0, mask_records(N, variant))
            t0 = time.perf_counter()
            res = run[call](r)
            ms = (time.perf_counter() - t0) * 1e3
            if variant in ("half", "unclipped"):
                info[f"{call}_{variant}_restored"] = r.mask_info(0)["restored"]
            info[f"{call}_written"] = res.get("written", res.get("filled"))
            return ms

        for call in CALLS:
            blocks = {k: [] for k in VARIANTS}
            for block in range(args.blocks):
                t = {k: [] for k in VARIANTS}
                for rep in range(args.reps + (1 if block == 0 else 0)):  # round 0 grows the buffers
                    turn += 1
                    for k in range(len(VARIANTS)):  # the variants take turns at going first
                        variant = VARIANTS[(k + turn) % len(VARIANTS)]
                        t[variant].append(one(call, variant))
                for k in VARIANTS:
                    blocks[k].append(float(np.median(t[k][1:] if block == 0 else t[k])))
            got[call] = {k: {"blocks": b, "median": float(np.median(b)), "spread": max(b) - min(b)} for k, b in blocks.items()}
        got["samples"], got["dab_at"], got["info"] = N ** 3, at, info
        for r in ctx.values():
            r.Stop()
        out[name] = got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
