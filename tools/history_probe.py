"""GPU probe (not part of the suite): what the edit history (vrt_volume_history) costs and what an undo is worth, on the demo's own
workload — workloads.voxelized_torus(8), the benched 256^3 voxelized-mesh volume (257^3 samples), made solid by the fill; one hard
SUBTRACT sphere dab of 8 cells on its surface — in both device formats.  Variants, alternating call by call:
  off_parent  the dab through the parent commit's library (--parent LIB, built beside this one with VRT_LIB_NAME), which has no history;
  off         the dab through this library with the history off: must cost what off_parent costs;
  on          the dab with the history on (capture, two compact passes, one record allocation), and then
  undo        vrt_volume_undo of that dab, against
  roundtrip   the only way back without a history, timed on the parent: vrt_volume_download_region of the dab's box before the edit plus
              vrt_volume_update_voxels of the same box after it (lossy on TEXEL16).
Every variant restores its volume after its dab, so every dab meets the same field; the three contexts take turns at going first.  Then the whole-grid case: vrt_volume_fill_enclosed
of the shell with the history off and on, and the bytes of the entry it records.  Times are host wall times around calls that end in a
synchronise.  The first round is not counted; a block is the median of --reps rounds, and the spread of the --blocks block medians
(max - min) is the run-to-run noise.  Prints one JSON line.

    python tools/history_probe.py --parent volumetricraytracer_amd/lib/libvrt_hip_parent.so [--reps 5] [--blocks 3] [--formats f32,texel16]
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

RADIUS = 8.0
BIG = (1 << 20, 1 << 40)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def load_parent(path):
    """The parent's library with the entry points it has (it lacks the history's)."""
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


def surface_sample(vol):
    """A sample of the shell about a quarter of the way through the grid's solid samples: the dab's centre, xyz."""
    solid = np.argwhere(np.asarray(vol.density) <= 0)
    x, z, y = solid[len(solid) // 4]
    return float(x), float(y), float(z)


class Variant:
    """One context holding the solid torus in slot 0, and the box a dab can write."""

    def __init__(self, lib, vol, history):
        self.r = renderer(lib)
        self.lib, self.ctx = self.r._lib, self.r._ctx
        self.r.upload_volume(0, vol)
        self.r.fill_enclosed(0, None, 1.0, 1)
        if history:
            self.r.enable_history(0, *BIG)
        c = surface_sample(vol)
        self.brush = (_abi.vrt_brush * 1)(v.sphere_brush(_abi.BRUSH_SUBTRACT, c, RADIUS, 0.0, 2.0, 0))
        reach = int(RADIUS + 2.0) + 1
        lo = [max(int(a) - reach, 0) for a in c]
        hi = [min(int(a) + reach, vol.N - 1) for a in c]
        self.origin = (C.c_int * 3)(*lo)
        self.size = (C.c_int * 3)(*[h - l + 1 for l, h in zip(lo, hi)])
        self.held = np.zeros(int(np.prod(list(self.size))), np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
        self.res = _abi.vrt_brush_result()

    def dab(self):
        _abi.check(self.lib.vrt_volume_apply_brushes(self.ctx, 0, 1, self.brush, C.byref(self.res)), "vrt_volume_apply_brushes")

    def download(self):
        _abi.check(self.lib.vrt_volume_download_region(self.ctx, 0, self.origin, self.size, self.held.ctypes.data_as(C.c_void_p)),
                   "vrt_volume_download_region")

    def update(self):
        _abi.check(self.lib.vrt_volume_update_voxels(self.ctx, 0, self.origin, self.size, self.held.ctypes.data_as(C.c_void_p)),
                   "vrt_volume_update_voxels")

    def undo(self):
        _abi.check(self.lib.vrt_volume_undo(self.ctx, 0, 1, None), "vrt_volume_undo")


def blocks_of(args, one_round):
    """one_round() -> {name: ms}; the block medians per name."""
    times = {}
    for block in range(args.blocks):
        t = {}
        for rep in range(args.reps + (1 if block == 0 else 0)):  # round 0 grows the buffers
            for k, ms in one_round().items():
                t.setdefault(k, []).append(ms)
        for k, ms in t.items():
            times.setdefault(k, []).append(float(np.median(ms[1:] if block == 0 else ms)))
    return {k: {"blocks": b, "median": float(np.median(b)), "spread": max(b) - min(b)} for k, b in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's library, built with VRT_LIB_NAME beside this one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--formats", default="f32,texel16")
    args = ap.parse_args()
    out = {"reps": args.reps, "blocks": args.blocks, "unit": "ms, median wall time around the calls, one value per block",
           "tile_bytes": _abi.HISTORY_TILE_BYTES, "dab_radius_cells": RADIUS}
    shell = workloads.voxelized_torus(8)
    for name in args.formats.split(","):
        vol = shell.set_device_format(_abi.FORMAT_TEXEL16 if name == "texel16" else _abi.FORMAT_F32)
        parent, off, on = Variant(load_parent(args.parent), vol, False), Variant(None, vol, False), Variant(None, vol, True)

        def by_parent(t):
            t["roundtrip_download"] = timed(parent.download)
            t["off_parent"] = timed(parent.dab)
            t["roundtrip_update"] = timed(parent.update)
            t["roundtrip"] = t["roundtrip_download"] + t["roundtrip_update"]

        def by_off(t):
            off.download()
            t["off"] = timed(off.dab)
            off.update()

        def by_on(t):
            t["on"] = timed(on.dab)
            t["undo"] = timed(on.undo)

        turn = [0]

        def one_round():  # the three take turns at going first, so that no variant always follows the same neighbour
            t = {}
            order = [by_parent, by_off, by_on]
            turn[0] += 1
            for k in range(3):
                order[(k + turn[0]) % 3](t)
            return t

        got = blocks_of(args, one_round)
        on.dab()
        info = on.r.history_info(0)
        on.undo()
        got.update(samples=vol.N ** 3, dab_written=int(on.res.written), dab_box_samples=int(np.prod(list(parent.size))),
                   dab_entry_tiles=info["top_tiles"], dab_entry_bytes=info["top_tiles"] * _abi.HISTORY_TILE_BYTES)
        for x in (parent, off, on):
            x.r.Stop()
        # the whole-grid case: the fill of the shell, history off and on (an upload empties the history and keeps it on)
        fills = {"fill_off": renderer(None), "fill_on": renderer(None)}
        for k, r in fills.items():
            r.upload_volume(0, vol)
            if k == "fill_on":
                r.enable_history(0, *BIG)

        def fill_round():
            t = {}
            for k, r in fills.items():
                r.upload_volume(0, vol)  # untimed
                t[k] = timed(lambda: r.fill_enclosed(0, None, 1.0, 1))
            return t

        got.update(blocks_of(args, fill_round))
        info = fills["fill_on"].history_info(0)
        got.update(fill_entry_tiles=info["top_tiles"], fill_entry_bytes=info["bytes"])
        for r in fills.values():
            r.Stop()
        out[name] = got
    print(json.dumps(out))


if __name__ == "__main__":
    main()
