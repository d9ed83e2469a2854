"""What the capacity scenes (capacity_scenes.py) have to contain for test_scene_capacity_gpu.py to mean anything, asserted on the
CPU oracle alone, and the Python mirror's own refusals at the limits of include/vrt.h.  These are conditions on the INPUTS (does a
ray really see 48 instances, does every one of the ten lights move pixels and cast a shadow, do the coincident twins really tie),
not measurements of the code under test: if a seed misses one, the scene's placement changes, never the figure.
Measured values: profiles/scene_capacity.txt."""
import copy

import numpy as np
import pytest

import capacity_scenes as cs
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi


@pytest.fixture(scope="module")
def oracle(oracle_lib):
    from oracle.binding import OracleScene

    return OracleScene


def _pixels(w=cs.W, h=cs.H):
    return [(x, y) for y in range(h) for x in range(w)]


def _camera_rays(osc, w=cs.W, h=cs.H):
    return osc.camera_rays(w, h, _pixels(w, h))


def _closest_instances(oracle, sc, p):
    """Per pixel of p's frame: the instance the oracle's camera ray hits first, -1 for a miss (OracleScene.trace, ray by ray)."""
    osc = oracle(sc)
    o, d = _camera_rays(osc, p.width, p.height)
    out = np.full(len(o), -1, np.int32)
    for k in range(len(o)):
        hit, _, _, inst, _ = osc.trace(p, o[k], d[k])
        if hit:
            out[k] = inst
    return out.reshape(p.height, p.width)


def _frame(oracle, sc, p):
    return oracle(sc).render(p, threads=8)


def _moved(a, b):
    return int((np.abs(a - b).max(axis=2) > 1e-3).sum())


@pytest.mark.parametrize("fmt", cs.LATTICE_FORMATS)
def test_lattice_shows_its_instances_and_every_volume(oracle, fmt):
    """>= 48 of the 64 instances are the closest hit of some camera ray at 96x54, all 20 volumes among them, and mirrors bounce."""
    sc = cs.lattice64(fmt)
    assert len(sc.Objects) == _abi.VRT_MAX_INSTANCES and len(sc.volumes()) == _abi.VRT_MAX_VOLUMES
    assert len(sc.PointLights) == _abi.VRT_MAX_POINT_LIGHTS and len(sc.SpotLights) == _abi.VRT_MAX_SPOT_LIGHTS
    resolutions = sorted(vol.Resolution for vol in sc.volumes())
    assert resolutions[0] == 3 and resolutions[-2:] == [4, 5]
    p = cs.params(sc, bounces=2)
    seen = np.unique(_closest_instances(oracle, sc, p))
    seen = seen[seen >= 0]
    vols = sc.volumes()
    slots = {next(i for i, vol in enumerate(vols) if vol is sc.Objects[k].Volume) for k in seen}
    _, st = _frame(oracle, sc, p)
    print(f"lattice64({fmt}): {len(seen)} instances seen, {len(slots)} volumes, bounce rays {st['bounce_rays']}, hits {st['hits']}")
    assert len(seen) >= 48
    assert slots == set(range(_abi.VRT_MAX_VOLUMES))
    assert st["bounce_rays"] > 0


@pytest.mark.parametrize("name", ["lattice64", "lights"])
def test_every_one_of_the_ten_lights_moves_pixels(oracle, name):
    """The oracle frame without light k differs from the full frame by more than 1e-3 in at least 30 pixels, for each of the ten."""
    sc = cs.lattice64("f32") if name == "lattice64" else cs.lights(5, 5)
    p = cs.params(sc, bounces=2)
    full, _ = _frame(oracle, sc, p)
    moved = [_moved(full, _frame(oracle, cs.without_light(sc, k), p)[0]) for k in range(10)]
    print(f"{name}: pixels moved by each light {moved}")
    assert min(moved) >= 30, moved


def test_every_light_of_the_light_scene_is_blocked_somewhere_and_seen_elsewhere(oracle):
    """lights(5, 5): for each light, >= 30 hit pixels whose shadow ray towards it (from 0.1 back along the camera ray, as the closest
    hit starts it) meets a surface before the light, and >= 30 where it does not.  (trace_batch takes one t_max for all rays: the
    rays run on, and `blocked` is a closest hit nearer than the light.)"""
    sc = cs.lights(5, 5)
    p = cs.params(sc)
    osc = oracle(sc)
    o, d = _camera_rays(osc)
    hit, t, _ = osc.trace_batch(p, o, d)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    start = (o + dn * t[:, None] - 0.1 * dn)[hit]
    assert len(start) >= 1000
    for k, L in enumerate(list(sc.PointLights) + list(sc.SpotLights)):
        to = np.asarray(L.Position, np.float32)[None, :] - start
        dist = np.linalg.norm(to, axis=1)
        h2, t2, _ = osc.trace_batch(p, start, to)
        blocked = h2 & (t2 < dist)
        print(f"light {k}: {int(blocked.sum())} pixels blocked, {int((~blocked).sum())} open")
        assert blocked.sum() >= 30 and (~blocked).sum() >= 30, k


@pytest.mark.parametrize("mode", [_abi.MODE_INTERP_NOTEX, _abi.MODE_CUBE_NOTEX])
@pytest.mark.parametrize("variant", ["two_volumes", "pairs32"])
def test_coincident_twins_show_the_lower_index(oracle, variant, mode):
    """The oracle's frame shows the material of the lower index in both orders (red or green), on at least 100 hit pixels, and the
    closest hit it reports is never the higher twin."""
    frames = {}
    for order in (0, 1):
        sc = cs.coincident(order, variant)
        p = cs.params(sc, mode=mode)
        img, st = _frame(oracle, sc, p)
        inst = _closest_instances(oracle, sc, p)
        hitpix = inst >= 0
        print(f"coincident({order}, {variant}) mode {mode}: {int(hitpix.sum())} hit pixels")
        assert hitpix.sum() >= 100 and st["hits"] >= 100
        if variant == "two_volumes":
            assert set(np.unique(inst[hitpix])) == {1}
        else:
            assert inst[hitpix].max() < 32 and len(np.unique(inst[hitpix])) >= 16
        r, g = img[..., 0][hitpix], img[..., 1][hitpix]
        lit = np.maximum(r, g) > 0.05
        assert lit.sum() >= 100
        assert np.all((r > g)[lit]) if order == 0 else np.all((g > r)[lit])
        frames[order] = img
    # one pixel, by name: where the first order's frame is reddest
    cy, cx = np.unravel_index(np.argmax(frames[0][..., 0] - frames[0][..., 1]), frames[0].shape[:2])
    assert frames[0][cy, cx, 0] - frames[0][cy, cx, 1] > 0.2 and frames[1][cy, cx, 1] - frames[1][cy, cx, 0] > 0.2


@pytest.mark.parametrize("order", [0, 1])
def test_shifted_twins_tie_bit_for_bit_in_a_cube_mode(oracle, order):
    """coincident(order, "shifted") in MODE_CUBE_NOTEX: each twin alone is hit by the same camera rays at bit-equal t (>= 100 of
    them), although their boxes differ; together the oracle reports the lower index, 1, everywhere."""
    sc = cs.coincident(order, "shifted")
    p = cs.params(sc, mode=_abi.MODE_CUBE_NOTEX)
    o, d = _camera_rays(oracle(sc))
    alone = []
    for k in (1, 3):
        one = copy.copy(sc)
        one.Objects = [sc.Objects[k]]
        alone.append(oracle(one).trace_batch(p, o, d))
    (hit1, t1, n1), (hit3, t3, n3) = alone
    assert hit1.sum() >= 100 and np.array_equal(hit1, hit3) and np.array_equal(t1, t3) and np.array_equal(n1, n3)
    lo, hi = cs.instance_boxes(sc)
    assert lo[3, 0] < lo[1, 0] and hi[3, 0] < hi[1, 0]
    inst = _closest_instances(oracle, sc, p)
    assert set(np.unique(inst[inst >= 0])) == {1} and (inst >= 0).sum() == hit1.sum()
    img, _ = _frame(oracle, sc, p)
    r, g = img[..., 0][inst >= 0], img[..., 1][inst >= 0]
    lit = np.maximum(r, g) > 0.05
    assert lit.sum() >= 50 and (np.all((r > g)[lit]) if order == 0 else np.all((g > r)[lit]))


def _boxes_met(o, d, lo, hi):
    """Per ray: how many of the boxes its line meets ahead of its origin — a plain float64 slab test."""
    o, d = np.asarray(o, np.float64)[:, None, :], np.asarray(d, np.float64)[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo[None] - o) / d, (hi[None] - o) / d
    te, tx = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
    return ((tx >= te) & (tx >= 0.0)).sum(axis=1)


@pytest.mark.parametrize("name", ["nested64:outside", "nested64:inside", "line64:0:along", "line64:0:back", "line64:0:diagonal", "line64:2:along"])
def test_nested_and_line_scenes_fill_the_frame_and_pierce_their_boxes(oracle, name):
    """>= 500 hit pixels each; line64 seen along the row: >= 200 camera rays whose direction meets 32 or more instance boxes; the
    camera of nested64's inside view lies in all 64 boxes."""
    kind, *args = name.split(":")
    sc = cs.nested64(args[0]) if kind == "nested64" else cs.line64(int(args[0]), args[1])
    assert len(sc.Objects) == 64
    p = cs.params(sc)
    osc = oracle(sc)
    o, d = _camera_rays(osc)
    hit, _, _ = osc.trace_batch(p, o, d)
    lo, hi = cs.instance_boxes(sc, np.float64)
    met = _boxes_met(o, d, lo, hi)
    print(f"{name}: {int(hit.sum())} hit pixels, rays through >= 32 boxes {int((met >= 32).sum())}, most boxes on a ray {int(met.max())}")
    assert hit.sum() >= 500
    if kind == "line64" and args[1] in ("along", "back"):
        assert (met >= 32).sum() >= 200
    if name == "nested64:inside":
        c = np.asarray(sc.Camera.Position, np.float64)
        assert np.all((lo < c) & (c < hi))
    if name == "nested64:outside":
        assert (met == 64).sum() >= 100  # rays that reach the innermost box: none of the 64 can be culled for them


@pytest.mark.parametrize("camera", cs.ODD_CAMERAS)
def test_odd_boxes_are_in_sight(oracle, camera):
    """near: the flat box, the turned cube and the torus are each the closest hit of >= 30 pixels; far: the distant sphere of >= 500,
    and its box's pad is about 10 units."""
    sc = cs.odd_boxes(camera)
    p = cs.params(sc)
    inst = _closest_instances(oracle, sc, p)
    counts = {k: int((inst == k).sum()) for k in range(4)}
    print(f"odd_boxes({camera}): closest-hit pixels per instance {counts}")
    if camera == "near":
        assert min(counts[0], counts[2], counts[3]) >= 30
    else:
        assert counts[1] >= 500
    lo, hi = cs.instance_boxes(sc)
    assert 9.9 < (hi[1, 0] - lo[1, 0] - 100.0) / 2 < 10.2
    assert hi[0, 2] - lo[0, 2] < 0.25


def test_the_python_mirror_refuses_what_the_abi_cannot_hold(oracle_lib):
    """VScene.to_abi(): 65 objects and 21 distinct volumes raise; of seven point and seven spot lights the first five are kept."""
    sc = copy.copy(cs.lattice64("f32"))
    sc.Objects = list(sc.Objects) + [sc.Objects[0]]
    with pytest.raises(ValueError):
        sc.to_abi()
    sc.Objects = list(cs.lattice64("f32").Objects[:40]) + [v.VVoxelObject(Volume=v.VVoxelVolume(1, 10.0))]
    with pytest.raises(ValueError):
        sc.to_abi()
    assert len(cs.lattice64("f32").to_abi().instances) == _abi.VRT_MAX_INSTANCES
    seven, five = cs.lights(7, 7), cs.lights(5, 5)
    assert len(seven.PointLights) == 7 and len(seven.SpotLights) == 7
    a, b = seven.to_abi(), five.to_abi()
    assert a.n_point_lights == 5 and a.n_spot_lights == 5
    assert bytes(a) == bytes(b)
