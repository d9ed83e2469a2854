"""Seeded sessions of volume calls in one context (tests/session_model.py): what a context carries from one call to the next — the
edit-report records, the scratch buffers that calls share and never clear, each slot's tables, active box, format and metric, the upload
format, the adaptor's own bookkeeping — is held to the model after EVERY step.  Each call's record is the model's; every device buffer of
both slots — dense grid, materials, bricks, cell records, both levels of the empty-space table, the Cube table and the active box —
equals volume_ref.device_bytes of the model's state; the slot a step does not name is byte-identical to what it was.  Tolerance 0; the
one exception is the frame against the oracle, within the suite's TOL.

Every test opens a context of its own, so the carried state starts cold and does not depend on the order of the files.  The coverage
conditions of the programs are asserted without a GPU, in tests/test_volume_session.py."""
import ctypes as C
import time

import numpy as np
import pytest

import session_model as M
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from oracle.binding import OracleScene
from test_volume_fill_gpu import TOL, assert_same_buffers, buffers, upload_field
from test_volume_mesh import assert_same_mesh
from test_volume_session import F32_SEED, SEEDS, programs, same_bits, what_of

pytestmark = pytest.mark.gpu


class DeviceSession:
    """The steps of a program on a context: through the C-ABI and the adaptor's thin calls, or — mirror — through the adaptor with a
    host volume passed to every call that takes one."""

    def __init__(self, r, mirror: bool = False):
        self.r, self.mirror = r, mirror
        self.vol = [None, None]   # mirror: the host volumes
        self.format = None        # what vrt_set_volume_format was last told: the context keeps it

    def _ptr(self, a):
        return np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)

    def _upload(self, slot, a):
        lib, ctx = self.r._lib, self.r._ctx
        if self.mirror:
            was = self.vol[slot]
            vol = v.VVoxelVolume(a["res"], a["extent"])
            if was is not None:  # the adaptor sends the volume's metric with every upload: a slot in use keeps its own
                vol.density_scale, vol.step_max = was.density_scale, was.step_max
            N = vol.N
            if a["path"] == "voxels":
                vol.density = np.array(a["records"]["density"].reshape(N, N, N))
                vol.material_id = np.array(a["records"]["material"].reshape(N, N, N))
            else:
                vol.density = np.array(a["density"])
                vol.material_id = np.array(a["material"]) if a["path"] == "float" else np.zeros((N, N, N), np.uint8)
            self.r.upload_volume(slot, vol, as_voxels=a["path"] == "voxels")
            self.vol[slot] = vol
            return
        if a["path"] != "texels" and a["fmt"] != self.format:  # an upload of texels is TEXEL16 whatever the context was told
            _abi.check(lib.vrt_set_volume_format(ctx, a["fmt"]), "vrt_set_volume_format")
            self.format = a["fmt"]
        head = (ctx, slot, a["res"], a["extent"])
        if a["path"] == "texels":
            rc = lib.vrt_volume_upload_texels(*head, self._ptr(a["texels"]))
        elif a["path"] == "voxels":
            rc = lib.vrt_volume_upload_voxels(*head, self._ptr(a["records"]))
        else:
            rc = lib.vrt_volume_upload(*head, self._ptr(a["density"]), self._ptr(a["material"]) if a["path"] == "float" else None)
        _abi.check(rc, "vrt_volume_upload*")

    def _update(self, slot, a):
        vol = self.vol[slot]
        (x0, y0, z0), (sx, sz, sy) = a["origin"], a["values"].shape
        if self.mirror:
            vol.set_region(a["origin"], a["values"], a["material"])
            self.r.update_volume_region(slot, vol, (x0, y0, z0), (x0 + sx - 1, y0 + sy - 1, z0 + sz - 1))
            return
        lib, ctx = self.r._lib, self.r._ctx
        origin, size = (C.c_int * 3)(x0, y0, z0), (C.c_int * 3)(sx, sy, sz)
        if a["records"]:
            rec = np.zeros(a["values"].shape, M.VOXEL)
            rec["density"], rec["material"] = a["values"], a["material"]
            rc = lib.vrt_volume_update_voxels(ctx, slot, origin, size, self._ptr(rec))
        else:
            rc = lib.vrt_volume_update_region(ctx, slot, origin, size, self._ptr(a["values"]),
                                              None if a["material"] is None else self._ptr(a["material"]))
        _abi.check(rc, "vrt_volume_update*")

    def apply(self, step):
        r, kind, slot, a = self.r, step["kind"], step["slot"], step["args"]
        vol = self.vol[slot]
        if kind == "upload":
            self._upload(slot, a)
        elif kind == "free":
            _abi.check(r._lib.vrt_volume_free(r._ctx, slot), "vrt_volume_free")
            r._uploaded.pop(slot, None)
            self.vol[slot] = None
        elif kind == "set_metric":
            _abi.check(r._lib.vrt_volume_set_metric(r._ctx, slot, a["scale"], a["step"]), "vrt_volume_set_metric")
            if vol is not None:
                vol.density_scale, vol.step_max = a["scale"], a["step"]
        elif kind == "update_region":
            self._update(slot, a)
        elif kind == "brushes":
            return r.apply_brushes(slot, vol, a["records"])
        elif kind == "stamp":
            return r.stamp_volume(slot, a["src"], a["record"], vol)
        elif kind == "smooth":
            return r.smooth_volume(slot, a["record"], vol)
        elif kind == "warp":
            return r.warp_volume(slot, a["record"], vol)
        elif kind == "fill":
            return r.fill_enclosed(slot, vol, a["wall"], a["material"])
        elif kind == "components":
            rec = _abi.components_record(a["op"], a.get("gap", 0.0), a.get("material_id", -1), a.get("min_samples", 0), a.get("seed", (0, 0, 0)))
            try:
                return r.components(slot, rec, vol, a["list_capacity"])
            except _abi.VrtError as e:
                assert e.status == _abi.VRT_ERR_INVALID
                return M.REFUSED
        elif kind == "redistance":
            return r.redistance(slot, vol, a["band"], a["from_"], a["lo"], a["hi"])
        elif kind == "extract_mesh":
            return r.extract_mesh(slot, a["iso"], a["lo"], a["hi"])
        elif kind == "download_region":
            return r.download_region(slot, a["lo"], a["hi"])
        elif kind == "download_volume":
            m = step["after"][slot]
            got = r.download_volume(slot, m.res, m.extent)
            return got.density, got.material_id
        else:
            raise AssertionError(kind)
        return None


def check_record(step, got, what):
    kind, want = step["kind"], step["want"]
    if kind == "extract_mesh":
        assert_same_mesh(got, want, what)
    elif kind in ("download_region", "download_volume"):
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    elif want is not None:
        assert M.same_record(kind, got, want), (what, got, want)


def slot_buffers(r, slot, used, device=0):
    """The slot's buffers, or None for a free slot — which the context must report as one."""
    if used:
        return buffers(r, slot, device)
    size = C.c_size_t(0)
    assert r._lib.vrt_debug_volume_bytes(r._ctx, slot, device, _abi.VOLUME_BYTES_DENSE, None, 0, C.byref(size)) == _abi.VRT_ERR_SLOT
    return None


def check_buffers(r, step, before, what, devices=(0,)):
    """Every buffer of both slots on every device against the model, and — the slot the step does not name, and every slot after a
    read-only step — against what it was.  Returns the buffers, for the next step."""
    now = {}
    for dev in devices:
        for slot in M.SLOTS:
            m = step["after"][slot]
            have = now[(dev, slot)] = slot_buffers(r, slot, m.used, dev)
            where = f"{what}: slot {slot} on device {dev}"
            if not m.used:
                continue
            assert_same_buffers(have, m.expected_buffers(), where + " against the model")
            if slot != step["slot"] or step["kind"] in M.READS:
                assert before[(dev, slot)] is not None, where
                assert_same_buffers(have, before[(dev, slot)], where + " against what it was")
    return now


def run_checked(r, seed, steps, devices=(0,), session=None, after_step=None):
    session = session or DeviceSession(r)
    before = {(dev, slot): None for dev in devices for slot in M.SLOTS}
    for step in steps:
        what = what_of(seed, step)
        got = session.apply(step)
        check_record(step, got, what)
        before = check_buffers(r, step, before, what, devices)
        if after_step:
            before = after_step(step, before, what) or before
    return session


@pytest.mark.parametrize("seed", SEEDS)
def test_every_step_of_a_session_holds_the_reference(seed):
    steps = M.program(seed)
    for step in steps:  # the model's share of the time, ahead of the device's
        for m in step["after"]:
            if m.used:
                m.expected_buffers()
    t0 = time.perf_counter()
    with v.VHipRenderer(devices=(0,)) as r:
        run_checked(r, seed, steps)
    print(f"seed {seed}: {len(steps)} steps and their checks on the device in {time.perf_counter() - t0:.2f} s")


def test_a_session_over_two_devices():
    """Smooth and warp among them: every step leaves both devices' copies of both slots as the model has them."""
    with v.VHipRenderer(devices=(0, 0)) as r:
        run_checked(r, SEEDS[0], M.program(SEEDS[0]), devices=(0, 1))


# ---- the adaptor and its host mirror -------------------------------------------------------------------------------------------------

def session_scene(vols):
    """Both slots' volumes side by side in front of config3's camera."""
    import math
    cam = v.VCamera(Position=(300.0 * math.cos(math.radians(35.0)), 0.0, 300.0 * math.sin(math.radians(35.0))),
                    Rotation=tuple(v.quat_mul(v.quat_from_axis_angle(v.UP, math.pi), v.quat_from_axis_angle(v.RIGHT, math.radians(35.0)))),
                    FOVAngle=60.0)
    objects = [v.VVoxelObject(Position=(0.0, -65.0 + 150.0 * slot, 0.0), Volume=vol) for slot, vol in enumerate(vols)]
    return v.VScene(Camera=cam, DirectionalLight=v.demo_light(), Objects=objects, EnvironmentMap=v.procedural_skybox(16))


def frame_params(sc):
    p = v.default_params(96, 54, min(vol.GetCellSize() for vol in sc.volumes()), 255, shadow=True)
    p.flags &= ~_abi.FLAG_NO_CULL_RECT  # a stale active box would show
    return p


def set_frame(r, sc, p):
    r.SetSceneToRender(sc)
    r.ResizeRenderOutput(p.width, p.height)
    r.params_override = p
    r.SetRendererMode(p.mode)


def test_the_mirror_follows_a_session():
    steps = M.program(F32_SEED, formats=(R.F32,))
    checkpoints = {10, 25, len(steps) - 1}
    with v.VHipRenderer(devices=(0,)) as r:
        session = DeviceSession(r, mirror=True)

        def after_step(step, before, what):
            for slot in M.SLOTS:
                m, vol = step["after"][slot], session.vol[slot]
                assert (vol is not None) == m.used, what
                if m.used:
                    assert same_bits(vol.density, m.stored) and np.array_equal(vol.material_id, m.material), f"{what}: the mirror of slot {slot}"
                    assert not vol.dirty and vol.dirty_box is None, f"{what}: the mirror of slot {slot} was dirtied"
            if step["n"] in checkpoints:  # a frame in between: nothing is sent again, nothing changes
                assert all(m.used for m in step["after"]), what
                sc = session_scene(session.vol)
                set_frame(r, sc, frame_params(sc))
                r.SyncWithScene()
                img = r.Render()
                assert img.shape == (54, 96, 4)
                for slot in M.SLOTS:
                    assert_same_buffers(buffers(r, slot), before[(0, slot)], f"{what}: slot {slot} after SyncWithScene and Render")
                checkpoints.discard(step["n"])

        run_checked(r, F32_SEED, steps, session=session, after_step=after_step)
    assert not checkpoints


# ---- what reads the volume after a session ---------------------------------------------------------------------------------------------

def final_volumes(steps):
    """Host volumes holding the model's final state: what a fresh context is given, and what the oracle marches."""
    vols = []
    for m in steps[-1]["after"]:
        vol = v.VVoxelVolume(m.res, m.extent).set_device_format(m.fmt)
        vol.density, vol.material_id = np.array(m.decoded()), np.array(m.material)
        vol.density_scale, vol.step_max = m.scale, m.step
        vols.append(vol)
    return vols


def adopt(r, vols):
    """The slots already hold the volumes: SyncWithScene has nothing to send."""
    for slot, vol in enumerate(vols):
        r._uploaded[slot] = id(vol)
        vol.dirty, vol.dirty_box = False, None


def read_everything(r, sc, p):
    set_frame(r, sc, p)
    frame = r.Render()
    w, h = p.width, p.height
    rays = r.camera_rays(np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="xy"), -1).reshape(-1, 2), w, h)
    hits = r.trace_rays(rays["origin"], rays["direction"], rays["t_max"], params=p)
    return frame, hits, [r.extract_mesh(slot) for slot in M.SLOTS]


@pytest.mark.parametrize("seed,kw", programs())
def test_what_reads_the_volume_after_a_session(oracle_lib, seed, kw):
    steps = M.program(seed, **kw)
    final = steps[-1]["after"]
    assert all(m.used for m in final)
    vols = final_volumes(steps)
    sc = session_scene(vols)
    p = frame_params(sc)
    with v.VHipRenderer(devices=(0,)) as r:
        session = DeviceSession(r)
        for step in steps:
            session.apply(step)
        adopt(r, vols)
        frame, hits, meshes = read_everything(r, sc, p)
    with v.VHipRenderer(devices=(0,)) as r:
        for slot, (m, vol) in enumerate(zip(final, vols)):
            upload_field(r, slot, vol, m.fmt, m.stored, m.material)  # one full upload and one set_metric
        adopt(r, vols)
        fresh_frame, fresh_hits, fresh_meshes = read_everything(r, sc, p)
    what = f"seed {seed}"
    assert same_bits(frame, fresh_frame), f"{what}: the frame differs in {int((frame.view(np.uint32) != fresh_frame.view(np.uint32)).sum())} values"
    for key in hits:
        a, b = hits[key], fresh_hits[key]
        assert same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b), (what, key)
    assert int(hits["hit"].sum()) > 200 and set(np.unique(hits["instance"][hits["hit"]])) == {0, 1}, what
    for slot in M.SLOTS:
        assert_same_mesh(meshes[slot], fresh_meshes[slot], f"{what}: the mesh of slot {slot}")
        assert_same_mesh(meshes[slot], final[slot].extract_mesh(), f"{what}: the mesh of slot {slot} against the model")
        assert meshes[slot][4]["vertices"] > 0
    if kw:  # F32: the oracle marches the mirror
        ref, _ = OracleScene(sc).render(p, threads=8)
        err = float(np.abs(frame - ref).max())
        print(f"{what}: max |frame - oracle| {err:.3e}")
        assert err <= TOL
