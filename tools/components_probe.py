"""GPU probe (not part of the suite): wall time of vrt_volume_components on the device — REPORT and REMOVE_SMALL — beside
vrt_volume_fill_enclosed on the same volume (the nearest existing labelling) and the host pass VVolumeConverter::Components, on
  solid  workloads.voxelized_torus(8), the benched 256^3 voxelized-mesh volume (257^3 samples), made solid by the fill: one component;
  specks tests/components_ref.specks_field(257): a solid sphere of 60 cells and some 230 specks, which REMOVE_SMALL takes out.
Ahead of every timed call the volume is uploaded again, outside the timed region, so every call meets the same field.  The first
round is not counted.  The timing block (--reps rounds, the median of each variant) is repeated --blocks times; the spread of the block
medians (max - min) is the run-to-run noise.  Prints one JSON line.

    python tools/components_probe.py [--reps 5] [--blocks 3] [--cases solid,specks] [--no-host]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volumetricraytracer_amd as v  # noqa: E402
from volumetricraytracer_amd import _abi  # noqa: E402
from volumetricraytracer_amd import voxelizer as vx  # noqa: E402
from volumetricraytracer_amd import workloads  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def case_volume(name):
    """(the volume as uploaded ahead of the fill's timing, the volume the components calls meet, REMOVE_SMALL's record)."""
    if name == "solid":
        shell = workloads.voxelized_torus(8)
        solid = copy.copy(shell)
        solid.density, solid.material_id = np.array(shell.density), np.array(shell.material_id)
        vx.fill_enclosed_host(solid, 1.0, 1)
        gap = 0.5 * solid.GetCellSize() / solid.density_scale
        return shell, solid, _abi.components_record(_abi.COMPONENTS_REMOVE_SMALL, gap, 0, 1000)
    import components_ref as CR
    d, m = CR.specks_field(257)
    vol = v.VVoxelVolume(8, 100.0)
    vol.density, vol.material_id = d, m
    vol.step_max = 1.5 * vol.GetCellSize()
    return vol, vol, _abi.components_record(_abi.COMPONENTS_REMOVE_SMALL, 0.5, 0, 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--cases", default="solid,specks")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    out = {"reps": args.reps, "blocks": args.blocks, "unit": "ms, median wall time around the call, one value per block", "format": "f32"}
    report = _abi.components_record(_abi.COMPONENTS_REPORT)
    with v.VHipRenderer() as r:
        for name in args.cases.split(","):
            before_fill, vol, small = case_volume(name)
            last = {}
            variants = {"report": (vol, lambda: last.__setitem__("report", r.components(0, report))),
                        "remove_small": (vol, lambda: last.__setitem__("remove_small", r.components(0, small))),
                        "fill_enclosed": (before_fill, lambda: last.__setitem__("fill_enclosed", r.fill_enclosed(0, None, 1.0, 1)))}
            times = {k: [] for k in variants}
            for block in range(args.blocks):
                t = {k: [] for k in variants}
                for rep in range(args.reps + (1 if block == 0 else 0)):  # round 0 grows the buffers
                    for k, (field, fn) in variants.items():
                        r.upload_volume(0, field)  # untimed
                        t[k].append(timed(fn))
                for k in variants:
                    times[k].append(float(np.median(t[k][1:] if block == 0 else t[k])))
            got = last["remove_small"]
            out[name] = {k: {"blocks": times[k], "median": float(np.median(times[k])), "spread": max(times[k]) - min(times[k])} for k in variants}
            out[name].update(samples=vol.N ** 3, components=got["components"], removed=got["removed"], written=got["written"],
                             solid=got["solid"], fill_filled=last["fill_enclosed"]["filled"], fill_rounds=last["fill_enclosed"]["sweeps"])
            if not args.no_host:
                host = []
                for rep in range(3):
                    work = copy.copy(vol)
                    work.density, work.material_id = np.array(vol.density), np.array(vol.material_id)
                    host.append(timed(lambda: vx.components_host(work, small)))
                out[name]["host_remove_small"] = {"runs": host, "median": float(np.median(host))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
