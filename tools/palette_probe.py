"""GPU box: what the palette's lookup costs — the painted sphere of tests/palette_ref.py at 1080p through the full closest hit in one
kernel, without a palette and with one, blocks of 48 frames in one launch, interleaved rounds."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
import palette_ref as pr

W, H, G = 1920, 1080, _abi.MAX_BLOCK_FRAMES
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
vol = pr.sphere_volume()
vol.Material = v.VMaterial(*pr.ENTRIES[0])
sc = pr.painted_sphere_scene(vol)
p = v.default_params(W, H, float(vol.GetCellSize()), 255, shadow=True, mode=_abi.MODE_INTERP_NOTEX)
p.flags = _abi.FLAG_FULL_ONE_KERNEL
r = v.VHipRenderer()
assert r.Start()
r.SetSceneToRender(sc)
r.ResizeRenderOutput(W, H)
r.SyncWithScene()
r.apply_brushes(0, vol, [pr.paint_record()])
buf = torch.empty((G, H, W, 4), dtype=torch.float32, device="cuda:0")


def run(n):
    for _ in range(n):
        r.render_block(p, G, buf.data_ptr(), H * W * 16, 0)
    torch.cuda.synchronize()


results = {"no palette": [], "palette": []}
for rnd in range(rounds):
    for name, entries in (("no palette", None), ("palette", pr.ENTRIES)):
        r.set_palette(0, entries)
        run(4)  # clocks ramp, buffers of this size exist: untimed
        t0 = time.perf_counter()
        run(8)
        dt = (time.perf_counter() - t0) / (8 * G)
        t = r.last_timing()
        form = r.last_kernel_form()
        assert bool(form & _abi.FORM_PALETTE) == (entries is not None) and form & _abi.FORM_FULL and not form & _abi.FORM_PASSES
        results[name].append(dt * 1e3)
        print(f"round {rnd + 1} {name:10s}: {dt * 1e3:.4f} ms/frame, hits {t['hits']}, rays {t['primary_rays'] + t['shadow_rays'] + t['bounce_rays']}")
a, b = results["no palette"], results["palette"]
ma, mb = sum(a) / len(a), sum(b) / len(b)
print(f"mean: no palette {ma:.4f} ms/frame (spread {max(a) - min(a):.4f}), palette {mb:.4f} ms/frame (spread {max(b) - min(b):.4f}): "
      f"{100.0 * (mb / ma - 1.0):+.2f} %")
r.Stop()
