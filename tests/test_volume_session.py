"""Seeded sessions of volume calls over two slots (tests/session_model.py) through the C++ host twins — vrh_stamp, vrh_smooth, vrh_warp,
vrh_fill_enclosed, vrh_components, vrh_redistance, vrh_extract_mesh, which compile the same *_core.h as the HIP kernels — with the model
of the context beside them: after every step the densities' bits, the ids and the reported record are the model's.  Tolerance 0.  This is
also the proof that the generator and the model are sound before tests/test_volume_session_gpu.py puts the same programs through a real
context, and where the coverage conditions of every seed that test uses are asserted.

What has no host twin runs as the package's host side does it: an upload stores the floats, or +-q by the package's own quantiser
(scene.texel16_q); a region update is VVoxelVolume.set_region; the brushes are the host pass tests/test_volume_brush.py has, the numpy
rule of tests/brush_ref.py.  The host fill knows the fp32 rule only: on a TEXEL16 slot it runs on the decoded densities and the samples
it filled are stored as their texels."""
import time

import numpy as np
import pytest

import brush_ref as B
import session_model as M
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx
from volumetricraytracer_amd.scene import texel16_q
from test_volume_mesh import assert_same_mesh

SEEDS = (0, 1, 2)  # the seeds of tests/test_volume_session_gpu.py
F32_SEED = 3       # its F32-only program: the host mirror can follow one


def same_bits(a, b) -> bool:
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def quantised(d, fmt):
    """What a slot of the format stores for the floats d, by the package's quantiser."""
    d = np.asarray(d, np.float32)
    if fmt == R.F32:
        return d.copy()
    q = texel16_q(d).astype(np.float32)
    return np.where(d < 0, -q, q).astype(np.float32)


class HostSession:
    """Two host volumes whose `density` is what the slot stores (+-q for a TEXEL16 slot), edited by the host twins."""

    def __init__(self):
        self.vol, self.fmt = [None, None], [None, None]

    def apply(self, step):
        kind, slot, a = step["kind"], step["slot"], step["args"]
        vol, fmt = self.vol[slot], self.fmt[slot]
        t16 = fmt == R.TEXEL16
        if kind == "upload":
            new = v.VVoxelVolume(a["res"], a["extent"])
            if vol is not None:  # a slot in use keeps its metric
                new.density_scale, new.step_max = vol.density_scale, vol.step_max
            if a["path"] == "texels":
                new.density, new.material_id = (np.array(x) for x in R.decode_texels(a["texels"]))
            elif a["path"] == "voxels":
                rec = a["records"]
                new.density = quantised(rec["density"].reshape((new.N,) * 3), a["fmt"])
                new.material_id = np.array(rec["material"].reshape((new.N,) * 3))
            else:
                new.density = quantised(a["density"], a["fmt"])
                new.material_id = np.array(a["material"]) if a["path"] == "float" else np.zeros((new.N,) * 3, np.uint8)
            self.vol[slot], self.fmt[slot] = new, a["fmt"]
        elif kind == "free":
            self.vol[slot] = self.fmt[slot] = None
        elif kind == "set_metric":
            vol.density_scale, vol.step_max = a["scale"], a["step"]
        elif kind == "update_region":
            vol.set_region(a["origin"], quantised(a["values"], fmt), a["material"])
        elif kind == "brushes":
            d, m = np.array(vol.density), np.array(vol.material_id)
            got = B.apply(d, m, fmt, a["records"], vol.VolumeExtends, vol.density_scale)
            vol.density, vol.material_id = d, m
            return got
        elif kind == "stamp":
            return vx.stamp_host(vol, self.vol[a["src"]], a["record"], t16, self.fmt[a["src"]] == R.TEXEL16)
        elif kind == "smooth":
            return vx.smooth_host(vol, a["record"], t16)
        elif kind == "warp":
            return vx.warp_host(vol, a["record"], t16)
        elif kind == "fill":
            if not t16:
                return vx.fill_enclosed_host(vol, a["wall"], a["material"])
            stored = np.array(vol.density)
            vol.density = B.decode(stored, fmt)
            got = vx.fill_enclosed_host(vol, a["wall"], a["material"])
            filled = vol.density.view(np.uint32) != B.decode(stored, fmt).view(np.uint32)
            assert int(filled.sum()) == got["filled"]
            vol.density = np.where(filled, quantised(vol.density, fmt), stored)
            return got
        elif kind == "components":
            rec = _abi.components_record(a["op"], a.get("gap", 0.0), a.get("material_id", -1), a.get("min_samples", 0), a.get("seed", (0, 0, 0)))
            try:
                return vx.components_host(vol, rec, t16, a["list_capacity"])
            except _abi.VrtError as e:
                assert e.status == _abi.VRT_ERR_INVALID
                return M.REFUSED
        elif kind == "redistance":
            return vx.redistance_host(vol, a["band"], a["from_"], a["lo"], a["hi"], texel16=t16)
        elif kind == "extract_mesh":
            return vx.extract_mesh_host(vol, a["iso"], a["lo"], a["hi"], texel16=t16)
        elif kind in ("download_region", "download_volume"):
            return None  # the device's calls: nothing on the host stands for them
        else:
            raise AssertionError(kind)
        return None


def what_of(seed, step):
    m = step["after"][step["slot"]]
    return f"seed {seed}, step {step['n']}: {step['kind']} on slot {step['slot']}" + (f" ({m.N}^3, format {m.fmt})" if m.used else "")


def run_host(seed, steps):
    host = HostSession()
    for step in steps:
        what = what_of(seed, step)
        got = host.apply(step)
        if step["kind"] == "extract_mesh":
            assert_same_mesh(got, step["want"], what)
        elif step["kind"] in M.EDITS and step["want"] is not None:
            assert M.same_record(step["kind"], got, step["want"]), (what, got, step["want"])
        for slot in M.SLOTS:
            m, vol = step["after"][slot], host.vol[slot]
            assert (vol is not None) == m.used, what
            if m.used:
                assert same_bits(vol.density, m.stored), f"{what}: densities of slot {slot}"
                assert np.array_equal(vol.material_id, m.material), f"{what}: ids of slot {slot}"
                assert (vol.N, vol.VolumeExtends, host.fmt[slot]) == (m.N, m.extent, m.fmt), what
                assert (vol.density_scale, vol.step_max) == (m.scale, m.step), what


def programs():
    return [(seed, {}) for seed in SEEDS] + [(F32_SEED, {"formats": (R.F32,)})]


@pytest.mark.parametrize("seed,kw", programs())
def test_the_host_twins_hold_the_model_through_a_session(seed, kw):
    t0 = time.perf_counter()
    M.program.cache_clear()  # the model's own time, whatever ran before
    steps = M.program(seed, **kw)
    t1 = time.perf_counter()
    run_host(seed, steps)
    t2 = time.perf_counter()
    print(f"seed {seed}: {len(steps)} steps, the model {t1 - t0:.2f} s, the host twins {t2 - t1:.2f} s")
    assert t1 - t0 < 10.0


@pytest.mark.parametrize("seed,kw", programs())
def test_the_programs_reach_what_they_are_for(seed, kw):
    steps = M.program(seed, **kw)
    cov = M.coverage(steps)
    print(f"seed {seed}: {cov}")
    assert M.shortfalls(cov) == []
    assert cov["steps"] == M.N_STEPS and set(cov["kinds"]) == set(M.KINDS)
    if not kw:
        assert "texels" in cov["upload_paths"] and {"float", "voxels", "float_nomat"} <= set(cov["upload_paths"])


def test_the_seeds_together_reach_every_choice():
    """What one program has no room for, the seeds share out: the four resolutions, the bands and modes of a redistance, the ops of a
    components call, the brushes' shapes and ops, the stamp's ops."""
    steps = [s for seed in SEEDS for s in M.program(seed)]
    of = lambda kind: [s for s in steps if s["kind"] == kind]
    assert {s["args"]["res"] for s in of("upload")} == {2, 3, 4, 5}
    assert {s["after"][s["slot"]].fmt for s in of("upload")} == {R.F32, R.TEXEL16}
    assert {s["args"]["band"] for s in of("redistance")} == set(M.BANDS) and {s["args"]["from_"] for s in of("redistance")} == set(M.FROMS)
    assert {s["args"]["op"] for s in of("components")} == {0, 1, 2, 3, 4}
    brushes = [r for s in of("brushes") for r in s["args"]["records"]]
    assert {(r.shape, r.op) for r in brushes} == {(shape, op) for shape in range(3) for op in range(3)}
    assert {s["args"]["record"].op for s in of("stamp")} == {0, 1, 2}
    assert {(s["after"][s["slot"]].fmt, s["after"][s["args"]["src"]].fmt) for s in of("stamp")} >= {(R.F32, R.TEXEL16), (R.TEXEL16, R.F32)}
    assert {s["args"]["record"].material for s in of("warp")} >= {-2, -1, 7}
    assert {s["args"]["step"] for s in of("set_metric")} >= {0.0, -1.0, float("inf")}
    assert {s["args"]["scale"] for s in of("set_metric")} == set(M.SCALES)


def test_the_model_of_an_upload_follows_the_slot_rule():
    """A slot in use keeps its metric through an upload; a freed one starts from (1, 0)."""
    rng = np.random.default_rng(5)
    d, ids = M.analytic_field(rng, 9, 60.0, "sphere")
    m = M.SlotModel()
    m.upload(3, 60.0, R.F32, "float", density=d, material=ids)
    assert (m.scale, m.step) == (1.0, 0.0) and m.expected_buffers()["active_box"] is None and m.expected_buffers()["skip"].size == 0
    m.set_metric(0.37, 7.5)
    assert m.expected_buffers()["skip"].size == 8  # two bricks per axis
    m.upload(2, 60.0, R.TEXEL16, "float_nomat", density=d[:5, :5, :5])
    assert (m.scale, m.step, m.N, m.fmt) == (0.37, 7.5, 5, R.TEXEL16) and not m.material.any()
    m.free()
    assert not m.used
    m.upload(3, 60.0, R.F32, "float", density=d, material=ids)
    assert (m.scale, m.step) == (1.0, 0.0)
