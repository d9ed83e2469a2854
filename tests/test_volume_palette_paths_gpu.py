"""Per-voxel materials on every instantiation of the full closest hit, and on what tests/test_volume_palette_gpu.py leaves unseen.  Each
test renders the palette frame P and the palette-free frames U_k (the slot's material = entry k), names every hit pixel's id with the
numpy restatement of the header's rule (tests/palette_ref.py) from the device's own closest hit and the volume as the device holds it,
and requires P == U_id bit for bit (palette_ref.check_composition); the U_k of the base scenes are held to the CPU oracle within the
parity tolerance, so that the chain ends at the independent reference.

  1. composition on the six kernel paths, with and without per-frame scenes (the DYN instantiations); which path runs follows
     resolve_path: F32 + PATH_BRICK -> VRT_PATH_BRICK; PATH_DENSE -> VRT_PATH_DENSE; every slot TEXEL16 + PATH_BRICK -> kPathBrick16,
     + PATH_CELLS -> kPathCells16; TEXEL16 beside F32 -> VRT_PATH_DENSE over a +-q field; a Cube mode -> kPathCube, every slot
     TEXEL16 -> kPathCube16
  2. the Cube modes: the seven-point criterion names the compared pixels; a hit renders the entered cell's nearest INSIDE sample, through
     low faces and through high ones
  3. three slots, four instances whose index is not their slot, two palettes of different lengths
  4. the mirror decision per pixel: only an entry mirrors; only the slot's own material mirrors
  5. the raw pair under a roughness / metallic texture
  6. a context of two devices
  7. -0 and +0 samples, F32 and TEXEL16, a palette of 256 entries and id 255
  and, beyond the list, step 3's other branch on many pixels: hits in cells without an INSIDE corner, outside samples with ids of their own

The twins of these scenes under the CPU oracle (tests/test_volume_palette.py) hold the same caps without a GPU."""
import numpy as np
import pytest

import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

import palette_ref as pr
from palette_ref import bits, camera_hits, check_composition, frame, material_of, uniform_frames, use

pytestmark = pytest.mark.gpu
ONE = _abi.FLAG_FULL_ONE_KERNEL


@pytest.fixture(scope="module")
def pal(oracle_lib):
    """A context of this module's own."""
    with v.VHipRenderer() as r:
        yield r


def palette_form(form):
    return bool(form & _abi.FORM_FULL) and bool(form & _abi.FORM_PALETTE) and not form & _abi.FORM_PASSES


def ids_on(r, sc, p, slot, inst, rays, got, which, cube_rule=False):
    """ids and boundary distances of the hits `which` (a mask over the pixels) on instance `inst`, from slot `slot` as the device holds
    it.  A Cube mode takes the seven-point criterion, or (cube_rule) the header's Cube-mode rule itself."""
    dv = r.download_volume(slot, pr.RESOLUTION, pr.EXTENT)
    obj = sc.Objects[inst]
    pts = pr.object_points(obj.Position, obj.Rotation, obj.Scale, rays["origin"][which], rays["direction"][which], got["t"][which])
    if cube_rule:
        return pr.entry_ids(dv.density, dv.material_id, pr.EXTENT, pts, pr.object_directions(obj.Rotation, obj.Scale, rays["direction"][which]))
    return pr.ids_of(dv.density, dv.material_id, p, pts)


def block_of_two(r, sc, p, P):
    """Two frames with their own scenes in one launch (the DYN instantiation): frame 0 is the scene, frame 1 has its object moved."""
    import torch

    arr = r.scene_array([sc, pr.moved(sc)])
    out = torch.zeros((2, p.height, p.width, 4), dtype=torch.float32, device="cuda")
    r.render_block(p, 2, out.data_ptr(), p.height * p.width * 16, 0, scenes=(arr, 0))
    torch.cuda.synchronize()
    assert palette_form(r.last_kernel_form())
    assert r.launch_history(1)[-1][1] == 2  # one launch covered both frames
    blk = out.cpu().numpy()
    assert np.array_equal(bits(blk[0]), bits(P))
    assert np.any(bits(blk[1]) != bits(P))  # the frame's own scene was rendered


# ---- 1. and 2. every instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.CASES))
def test_composition_on_every_path_and_with_per_frame_scenes(pal, name):
    r = pal
    sc, p, vol = pr.case_scene(name, flags=ONE)
    use(r, sc, p)
    U = uniform_frames(r, vol, pr.ENTRIES, oracle=(sc, p))
    r.set_palette(0, pr.ENTRIES)
    P, _, form = frame(r)
    assert palette_form(form)
    rays, got = camera_hits(r, p)
    on = got["hit"] & (got["instance"] == 0)
    ids, dist = ids_on(r, sc, p, 0, 0, rays, got, on)
    check_composition(P, U, ids, dist, np.flatnonzero(on), int(on.sum()), cap=pr.excluded_cap(p), what=f"{name}: ")
    rest = ~on
    for k in range(3):  # the sky and a second object: the same in every frame
        assert np.array_equal(bits(P).reshape(-1, 4)[rest], bits(U[k]).reshape(-1, 4)[rest])
    assert np.any(bits(U[1]) != bits(U[2])) and np.any(bits(U[0]) != bits(U[1]))
    if len(sc.Objects) > 1:
        assert int((got["hit"] & (got["instance"] == 1)).sum()) > 50  # the second object shows
    block_of_two(r, sc, p, P)
    r.set_palette(0, None)


@pytest.mark.parametrize("name", ["cube", "cube16"])
def test_a_cube_hit_renders_the_entered_cell(pal, name):
    """From +Y the rays enter most solid cells through a HIGH face, beyond which the cell before has no INSIDE corner: the header's Cube
    rule names the entered cell, the restatement follows it, and the cell it names is solid (its own sample INSIDE) at every hit."""
    r = pal
    sc, p, vol = pr.case_scene(name, flags=ONE, cube_view=None)
    use(r, sc, p)
    U = uniform_frames(r, vol, pr.ENTRIES)
    r.set_palette(0, pr.ENTRIES)
    P, _, form = frame(r)
    assert palette_form(form)
    rays, got = camera_hits(r, p)
    hit = got["hit"]
    ids, dist = ids_on(r, sc, p, 0, 0, rays, got, hit, cube_rule=True)
    ok = check_composition(P, U, ids, dist, np.flatnonzero(hit), int(hit.sum()), what=f"{name}, the entered cell: ")
    assert int((ids == 0).sum()) == 0  # an entered cell has an INSIDE corner: never the nearest-sample fallback
    obj = sc.Objects[0]
    pts = pr.object_points(obj.Position, obj.Rotation, obj.Scale, rays["origin"][hit], rays["direction"][hit], got["t"][hit])
    od = pr.object_directions(obj.Rotation, obj.Scale, rays["direction"][hit])
    _, c, _ = pr.hit_cells(vol.N, pr.EXTENT, pts, od)
    dv = r.download_volume(0, pr.RESOLUTION, pr.EXTENT)
    assert np.all(dv.density[c[ok, 0], c[ok, 2], c[ok, 1]] <= 0)
    high = np.any((np.abs(pts + pr.EXTENT - np.round(pts + pr.EXTENT)) < 1e-3) & (od < 0), axis=1)  # (cells of 1.0)
    print(f"{name}: {int(high.sum())} of {int(hit.sum())} hits entered through a high face")
    assert int(high.sum()) > 0.5 * int(hit.sum())
    r.set_palette(0, None)


def test_without_an_inside_corner_the_nearest_sample_names_the_entry(pal):
    """Step 3's other branch, on enough pixels to matter: seen from far away a good part of the hits stop in the cell outside the surface,
    and the outside samples carry ids of their own here, differing between neighbours — the cell's corner 0 is not the nearest sample."""
    r = pal
    sc, p, vol = pr.far_scene(flags=ONE)
    use(r, sc, p)
    U = uniform_frames(r, vol, pr.ENTRIES, oracle=(sc, p))
    r.set_palette(0, pr.ENTRIES)
    P, _, form = frame(r)
    assert palette_form(form)
    rays, got = camera_hits(r, p)
    hit = got["hit"]
    ids, dist = ids_on(r, sc, p, 0, 0, rays, got, hit)
    ok = check_composition(P, U, ids, dist, np.flatnonzero(hit), int(hit.sum()), what="far: ")
    dv = r.download_volume(0, pr.RESOLUTION, pr.EXTENT)
    obj = sc.Objects[0]
    pts = pr.object_points(obj.Position, obj.Rotation, obj.Scale, rays["origin"][hit], rays["direction"][hit], got["t"][hit])
    bare, corner0 = pr.without_inside_corner(dv.density, dv.material_id, pr.EXTENT, pts)
    print(f"far: {int((bare & ok).sum())} compared hits in a cell without an INSIDE corner, corner 0 of another id on {int((bare & ok & (corner0 != ids)).sum())}")
    assert int((bare & ok).sum()) >= 50 and int((bare & ok & (corner0 != ids)).sum()) >= 20
    r.set_palette(0, None)


# ---- 3. slots, instances and two palettes --------------------------------------------------------------------------------------------
def test_instances_take_the_palette_of_their_own_slot(pal):
    r = pal
    sc, p, vols = pr.slots_scene()
    p.flags = ONE
    use(r, sc, p)
    B3 = pr.PALETTE_B + (pr.SLOT2_OWN,)  # id 2 is beyond palette B: slot 2's own material
    U = uniform_frames(r, vols[1], pr.PALETTE_A, also=[(vols[2], B3)], oracle=(sc, p))
    r.set_palette(1, pr.PALETTE_A)
    r.set_palette(2, pr.PALETTE_B)
    assert len(r.get_palette(0)) == 0 and len(r.get_palette(1)) == 3 and len(r.get_palette(2)) == 2
    P, t, form = frame(r)
    assert palette_form(form) and t["bounce_rays"] == 0
    rays, got = camera_hits(r, p)
    for i, slot in enumerate(pr.SLOTS_INSTANCES):
        on = got["hit"] & (got["instance"] == i)
        assert int(on.sum()) > 100, i
        if slot == 0:  # no palette: the same pixels in every frame
            for k in range(3):
                assert np.array_equal(bits(P).reshape(-1, 4)[on], bits(U[k]).reshape(-1, 4)[on])
            continue
        ids, dist = ids_on(r, sc, p, slot, i, rays, got, on)
        check_composition(P, U, ids, dist, np.flatnonzero(on), int(on.sum()), what=f"instance {i} (slot {slot}): ")
    for slot in (1, 2):
        r.set_palette(slot, None)


# ---- 4. the mirror decision per pixel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["entry", "slot"])
def test_the_bounce_is_decided_by_the_surface_of_the_pixel(pal, which):
    r = pal
    sc, p, vol = pr.bounce_scene()
    use(r, sc, p)
    if which == "entry":  # (a) only an entry mirrors
        palette, entries, mirror_id = pr.ONLY_AN_ENTRY_MIRRORS, pr.ONLY_AN_ENTRY_MIRRORS, 1
    else:                 # (b) only the slot's own material mirrors, which id 2 falls back to
        vol.Material = material_of(pr.SLOT_MIRROR)
        palette, entries, mirror_id = pr.ONLY_THE_SLOT_MIRRORS, pr.ONLY_THE_SLOT_MIRRORS + (pr.SLOT_MIRROR,), 2
    tU = []
    U = uniform_frames(r, vol, entries, oracle=(sc, p), timings=tU)
    assert tU[0]["bounce_rays"] == 0 and tU[mirror_id]["bounce_rays"] > 0
    r.set_palette(0, palette)
    P, t, form = frame(r)
    assert palette_form(form) and form & _abi.FORM_MAY_BOUNCE
    rays, got = camera_hits(r, p)
    on = got["hit"] & (got["instance"] == 0)
    assert int((got["hit"] & (got["instance"] == 1)).sum()) > 50
    ids, dist = ids_on(r, sc, p, 0, 0, rays, got, on)
    ok = check_composition(P, U, ids, dist, np.flatnonzero(on), int(on.sum()), what=f"only the {which} mirrors: ")
    assert tU[mirror_id]["bounce_rays"] == int(on.sum())  # the whole sphere a mirror: one bounce a pixel, no reflected ray returns to it
    c, x = int((ok & (ids == mirror_id)).sum()), int((~ok).sum())
    print(f"only the {which} mirrors: bounce rays {t['bounce_rays']}, compared pixels of id {mirror_id}: {c}, excluded {x}; U_{mirror_id}: {tU[mirror_id]['bounce_rays']}")
    assert c <= t["bounce_rays"] <= c + x  # the sphere is convex: one bounce for every pixel whose surface mirrors, none elsewhere
    r.set_palette(0, None)


# ---- 5. the raw pair -------------------------------------------------------------------------------------------------------------------
def test_the_raw_pair_under_a_roughness_metallic_texture(pal):
    r = pal
    sc, p, vol = pr.textured_scene()
    use(r, sc, p)
    tU = []
    U = uniform_frames(r, vol, pr.ENTRIES, timings=tU)
    # the texture takes entry 2's roughness, 0.35, across 0.3 and none of the others'
    assert tU[0]["bounce_rays"] == 0 and tU[1]["bounce_rays"] == 0 and tU[2]["bounce_rays"] > 0
    r.set_palette(0, pr.ENTRIES)
    P, t, form = frame(r)
    assert palette_form(form) and form & _abi.FORM_TEXTURED
    rays, got = camera_hits(r, p)
    hit = got["hit"]
    ids, dist = ids_on(r, sc, p, 0, 0, rays, got, hit)
    check_composition(P, U, ids, dist, np.flatnonzero(hit), int(hit.sum()), what="textured, raw pair: ")
    print(f"textured: bounce rays {t['bounce_rays']} (U_2: {tU[2]['bounce_rays']})")
    assert 0 < t["bounce_rays"] < tU[2]["bounce_rays"]
    r.set_palette(0, None)


# ---- 6. every device of the context --------------------------------------------------------------------------------------------------
def test_a_context_of_two_devices_renders_the_one_device_frames(pal):
    sc, p, vol = pr.case_scene("brick", flags=ONE)
    use(pal, sc, p)
    base, _, _ = frame(pal)
    pal.set_palette(0, pr.ENTRIES)
    one, _, form = frame(pal)
    assert palette_form(form) and np.any(bits(one) != bits(base))
    pal.set_palette(0, None)
    with v.VHipRenderer(devices=(0, 0)) as r:
        use(r, sc, p)
        r.set_palette(0, pr.ENTRIES)
        two, _, form = frame(r)
        assert palette_form(form)
        assert np.array_equal(bits(two), bits(one))
        r.set_palette(0, None)
        off, _, form = frame(r)
        assert not form & _abi.FORM_PALETTE
        assert np.array_equal(bits(off), bits(base))
    vol.dirty = True  # (the module's context meets this volume anew)


# ---- 7. zeros and the last id ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [_abi.FORMAT_F32, _abi.FORMAT_TEXEL16])
def test_zeros_of_both_signs_are_inside_and_id_255_is_an_entry(pal, fmt):
    r = pal
    sc, p, vol = pr.zeros_scene(fmt)
    use(r, sc, p)
    dv = r.download_volume(0, pr.RESOLUTION, pr.EXTENT)
    band = np.abs(pr.sphere_volume().density) < np.float32(pr.ZERO_BAND)
    i = np.arange(vol.N)
    odd = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) & 1) == 1
    assert np.all(dv.density[band] == 0) and np.array_equal(np.signbit(dv.density[band]), odd[band])  # the device holds -0 and +0
    assert odd[band].any() and (~odd[band]).any() and np.array_equal(dv.material_id, vol.material_id)
    palette = pr.zeros_palette()
    rays, got = camera_hits(r, p)
    hit = got["hit"]
    ids, dist = ids_on(r, sc, p, 0, 0, rays, got, hit)
    occur = sorted(set(ids.tolist()))
    assert set(pr.ZERO_IDS) <= set(occur) and len(occur) <= 6
    U = dict(zip(occur, uniform_frames(r, vol, [palette[k] for k in occur])))
    r.set_palette(0, palette)
    assert len(r.get_palette(0)) == 256
    P, _, form = frame(r)
    assert palette_form(form)
    ok = check_composition(P, U, ids, dist, np.flatnonzero(hit), int(hit.sum()), need=pr.ZERO_IDS, what=f"zeros, format {fmt}: ")
    assert int((ok & (ids == 255)).sum()) >= 20
    assert np.any(bits(U[255]) != bits(U[254]))
    r.set_palette(0, None)
