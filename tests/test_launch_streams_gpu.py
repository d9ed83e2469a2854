"""What a launch stream owns (csrc/vrt_context.h, LaunchStream: per-wave counters, camera records, scene sections, hit records) when
more streams launch than there are records: the stream beyond the sixteenth takes over the least recently used record, a captured
launch outlives the take-over of its record, hit records and camera records change hands without reaching a pixel — and the
refusals of the render entry points, each with its code and without a trace in vrt_last_timing."""
import copy
import ctypes as C

import numpy as np
import pytest

from volumetricraytracer_amd import workloads as scenes
import volumetricraytracer_amd as v
from oracle.binding import OracleScene
from volumetricraytracer_amd import _abi

from test_parity_gpu import STAT_KEYS, TOL, _orbit

pytestmark = pytest.mark.gpu
RECORDS = 16  # csrc/vrt_context.h, kStatSlots
OTHERS = RECORDS + 1  # fresh streams that, launched on in turn, push every earlier stream out of its record


def _use(renderer, sc, W, H):
    renderer.SetSceneToRender(sc)
    renderer.ResizeRenderOutput(W, H)
    renderer.SyncWithScene()
    return v.default_params(W, H, scenes.min_cell(sc), 255, shadow=True)


def _lit_torus():
    """test_full_closest_hit_in_passes_on_two_streams_at_once's scene: one point light, so a block runs the full closest hit in passes."""
    sc = scenes.config3_torus(6, 32)
    sc.PointLights = [v.VPointLight(Position=(150.0, 40.0, 120.0), IlluminationStrength=400.0, Color=(1.0, 0.8, 0.6, 1.0),
                                    AttenuationLinear=0.05, AttenuationExp=0.002)]
    return sc


def test_a_stream_beyond_the_sixteenth_takes_over_the_oldest_record(renderer, oracle_lib):
    """Stream A, 17 fresh streams, A again: every frame is the first one, and after every launch vrt_last_timing reads the counters of
    that launch (through the record its stream holds now)."""
    import torch

    sc = scenes.config3_torus(6, 16)
    W, H = 64, 40
    p = _use(renderer, sc, W, H)
    ref, st = OracleScene(sc).render(p, threads=8)
    first = None
    a = torch.cuda.Stream()
    for k, stream in enumerate([a] + [torch.cuda.Stream() for _ in range(OTHERS)] + [a]):
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        with torch.cuda.stream(stream):
            renderer.render_rows(p, 0, H, out.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        t = renderer.last_timing()
        assert t["primary_steps"] == st["primary_steps"] and t["hits"] == st["hits"] > 0, k
        if first is None:
            first = out
        assert torch.equal(out, first), k
    assert np.abs(first.cpu().numpy() - ref).max() <= TOL


def test_a_captured_launch_survives_the_take_over_of_its_record(renderer, oracle_lib):
    """A frame captured on stream A replays the direct launch's pixels after 17 other streams have launched a larger frame: A's record
    has gone to another stream and its counter buffer was outgrown there — retired, not freed."""
    import torch

    sc = scenes.config3_torus(6, 16)
    W, H = 64, 40
    p = _use(renderer, sc, W, H)
    a = torch.cuda.Stream()
    direct = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(a):
        renderer.render_rows(p, 0, H, direct.data_ptr(), a.cuda_stream)  # the one warm-up launch of that size on the stream
    torch.cuda.synchronize()
    out = torch.zeros_like(direct)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=a):
        renderer.render_rows(p, 0, H, out.data_ptr(), a.cuda_stream)
    assert float(out.abs().max()) == 0.0 and float(direct.abs().max()) > 0.0  # capture does not execute
    big = v.default_params(2 * W, 2 * H, scenes.min_cell(sc), 255, shadow=True)
    bigbuf = torch.zeros((2 * H, 2 * W, 4), dtype=torch.float32, device="cuda:0")
    for stream in [torch.cuda.Stream() for _ in range(OTHERS)]:
        with torch.cuda.stream(stream):
            renderer.render_rows(big, 0, 2 * H, bigbuf.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, direct)


def test_hit_records_and_camera_records_across_a_take_over(renderer, oracle_lib):
    """The records that decide pixels: a 2-frame block (the full closest hit in passes: hit records), then a 49-frame block (cameras
    in device memory: camera records), each on 18 streams in turn — the first stream's block, bit for bit, every time."""
    import torch

    sc = _lit_torus()
    W, H = 32, 16
    p = _use(renderer, sc, W, H)
    assert 49 > _abi.MAX_BLOCK_FRAMES
    sf = copy.copy(sc)
    cam0 = _orbit(sc.Camera, 1)[0]
    sf.Camera = v.VCamera(Position=cam0[0], Rotation=cam0[1], FOVAngle=cam0[2])
    ref, _ = OracleScene(sf).render(p, threads=8)
    for n in (2, 49):
        cams = renderer.camera_array(_orbit(sc.Camera, n))
        first = None
        for k, stream in enumerate([torch.cuda.Stream() for _ in range(RECORDS + 2)]):
            block = torch.zeros((n, H, W, 4), dtype=torch.float32, device="cuda:0")
            with torch.cuda.stream(stream):
                renderer.render_block(p, n, block.data_ptr(), H * W * 16, stream.cuda_stream, cameras=(cams, 0), rows=(0, H))
            torch.cuda.synchronize()
            if first is None:
                first = block
                assert [fr for _, fr in renderer.launch_history(1)] == [n]
                assert bool(renderer.last_kernel_form() & _abi.FORM_PASSES)
                assert not torch.equal(block[0], block[n - 1])
            assert torch.equal(block, first), (n, k)
            assert np.abs(block[0].cpu().numpy() - ref).max() <= TOL, (n, k)


def test_refusals_are_what_they_were(renderer, oracle_lib):
    """Invalid arguments of the four render entry points, each with the code it returns; a refused call launches nothing and
    vrt_last_timing goes on reporting the last good launch."""
    import torch

    sc = scenes.config3_torus(6, 16)
    W, H = 64, 40
    p = _use(renderer, sc, W, H)
    lib, ctx = _abi.load(), renderer._ctx
    buf = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
    renderer.render_rows(p, 0, H, buf.data_ptr(), 0)
    torch.cuda.synchronize()
    keep = ("width", "height") + STAT_KEYS
    good = {k: renderer.last_timing()[k] for k in keep}
    assert good["hits"] > 0
    ptr, null, frame = C.c_void_p(buf.data_ptr()), C.c_void_p(), H * W * 16
    INVALID, UNSUPPORTED = _abi.VRT_ERR_INVALID, _abi.VRT_ERR_UNSUPPORTED
    rgba8 = _abi.vrt_params.from_buffer_copy(p)
    rgba8.flags |= _abi.FLAG_OUTPUT_RGBA8
    three = _abi.vrt_params.from_buffer_copy(p)
    three.flags |= _abi.FLAG_FULL_THREE_PASS
    two_scenes = renderer.scene_array([sc, sc])
    two_cameras = renderer.camera_array(_orbit(sc.Camera, 2))

    def rows(row0, n, out):
        return lib.vrt_render_rows(ctx, C.byref(p), row0, n, out, None)

    def strips(strip_rows, first, stride, n, out):
        return lib.vrt_render_strips(ctx, C.byref(p), strip_rows, first, stride, n, out, None)

    def block(params=p, out=ptr, **fields):
        b = _abi.vrt_block()
        b.n_frames, b.rows, b.frame_stride_bytes = 2, H, frame
        for name, value in fields.items():
            setattr(b, name, value)
        return lib.vrt_render_block(ctx, C.byref(params), C.byref(b), out, None)

    def block_host(out):
        b = _abi.vrt_block()
        b.n_frames, b.rows = 2, H
        return lib.vrt_render_block_host(ctx, C.byref(p), C.byref(b), out)

    scenes_ptr = C.cast(two_scenes, C.POINTER(_abi.vrt_scene))
    table = [
        ("rows: row0 < 0", lambda: rows(-1, 8, ptr), INVALID),
        ("rows: row0 + rows > height", lambda: rows(H - 7, 8, ptr), INVALID),
        ("rows: no buffer", lambda: rows(0, 8, null), INVALID),
        ("strips: strip_rows 0", lambda: strips(0, 0, 1, 1, ptr), INVALID),
        ("strips: first_strip >= strip_stride", lambda: strips(8, 2, 2, 1, ptr), INVALID),
        ("strips: n_strips * strip_rows > 16384", lambda: strips(8, 0, 1, 2049, ptr), INVALID),
        ("strips: no buffer", lambda: strips(8, 0, 1, 1, null), INVALID),
        ("block: n_frames 0", lambda: block(n_frames=0), INVALID),
        ("block: n_frames 257", lambda: block(n_frames=_abi.MAX_LAUNCH_FRAMES + 1), INVALID),
        ("block: strip_rows < 0", lambda: block(strip_rows=-1), INVALID),
        ("block: stride smaller than a frame", lambda: block(frame_stride_bytes=frame - 16), INVALID),
        ("block: stride no multiple of a float pixel", lambda: block(frame_stride_bytes=frame + 8), INVALID),
        ("block: stride no multiple of an RGBA8 pixel", lambda: block(params=rgba8, frame_stride_bytes=H * W * 4 + 2), INVALID),
        ("block: scenes together with cameras",
         lambda: block(scenes=scenes_ptr, cameras=C.cast(two_cameras, C.POINTER(_abi.vrt_camera))), INVALID),
        ("block_host: no host_frames", lambda: block_host(None), INVALID),
    ]
    with_palette = [
        ("block: three passes over a palette scene", lambda: block(params=three), UNSUPPORTED),
        ("block: three passes over per-frame scenes with a palette", lambda: block(params=three, scenes=scenes_ptr), UNSUPPORTED),
    ]

    def run(cases):
        for what, call, code in cases:
            assert call() == code, what
            assert {k: renderer.last_timing()[k] for k in keep} == good, what

    run(table)
    renderer.set_palette(0, [((0.5, 0.5, 0.5, 1.0), 0.5, 0.0)] * 2)
    try:
        run(with_palette)
    finally:
        renderer.set_palette(0, None)
    torch.cuda.synchronize()
    assert float(buf[1].abs().max()) == 0.0  # nothing was launched: no call reached the second frame of the buffer
    assert block() == _abi.VRT_OK  # the table's block, left as it is, is a good one
    torch.cuda.synchronize()
    assert torch.equal(buf[1], buf[0]) and {k: renderer.last_timing()[k] for k in keep} == good
