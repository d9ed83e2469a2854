"""The CPU converter (VVolumeConverter::ConvertMeshInfoToVoxelVolume, built from csrc/voxelize_core.h like the device kernel) against
the independent float64 reference of tests/voxelize_ref.py, over the WHOLE grid: near voxels, the far values inside a triangle's
box, the background outside every box, with triangles that the clip cuts, thins to one voxel or leaves out entirely.

Well-conditioned input is pinned to the reference within the derived tolerance (voxelize_ref.tol).  Needles, sub-cell triangles,
duplicated faces and damaged vertices cannot be pinned to float64; for them the properties that hold whatever the rounding are
asserted.  Each test prints its worst error in units of (N-1) * 2^-23 (the tolerance is 4): profiles/voxelize_reference.txt."""
import re

import numpy as np
import pytest

import voxelize_ref as V
from volumetricraytracer_amd import voxelizer as vx

SOUP_RESOLUTIONS = (0, 1, 2, 3, 4, 5, 6)
ILL_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
ILL_RESOLUTIONS = (4, 5, 6)


def soups(resolutions):
    """The three soups at every resolution; at resolution 0 a triangle of span 0.15 * extent cannot have an edge of cell/4 = 0.5 extent,
    so the 300-triangle soup starts at resolution 1."""
    return [(res, n, span) for res in resolutions for n, span in V.SOUPS if not (res == 0 and span < 1.0)]


def well_cases(resolutions=SOUP_RESOLUTIONS, others=(1, 4, 6)):
    """name -> builder of every well-conditioned case."""
    out = {f"soup_{n}_{span}_res{res}": (lambda res=res, n=n, span=span: V.clipped_soup(res, n, span)) for res, n, span in soups(resolutions)}
    for res in others:
        out[f"outside_far_res{res}"] = lambda res=res: V.outside_only(res, False)
        out[f"outside_near_res{res}"] = lambda res=res: V.outside_only(res, True)
    out["small_extent_res6"] = V.small_extent
    return out


WELL = well_cases()


def cpu_twin(case: V.Case, capfd=None):
    """The CPU converter on a case, with bounds chosen so that 1.25 * max = extent; (volume, skipped or None): the converter reports
    what it skipped in a warning on stdout only."""
    be = np.float32(case.extent) * np.float32(0.8)
    if capfd is not None:
        capfd.readouterr()
    vol = vx.convert_mesh(case.positions, case.indices, (be, be, be), f"case_{case.resolution}")
    assert vol.Resolution == case.resolution and vol.VolumeExtends == np.float32(case.extent)
    N, cell, thr = V.grid(case.resolution, case.extent)
    assert vol.N == N and np.float32(vol.GetCellSize()) == np.float32(cell) and np.float32(vol.density_scale) == np.float32(thr)
    skipped = None
    if capfd is not None:
        found = re.findall(r"Skipped (\d+) degenerate", capfd.readouterr().out)
        skipped = int(found[0]) if found else 0
    return vol, skipped


def check_well(case: V.Case, density, material, who: str):
    """A whole grid against the reference of a well-conditioned case: densities within tol, background exact, materials wherever the
    reference's density is further than tol from 0 (at most 0.1 % of the voxels are not)."""
    N = V.grid(case.resolution, case.extent)[0]
    exp = V.expected(case)
    want = exp.ref.density
    assert exp.ref.ambiguous == 0
    assert density.dtype == np.float32 and density.shape == want.shape
    err = V.scaled_error(N, density, want)
    print(f"voxelize_reference: {case.name:28s} {who:6s} worst scaled error {err:.3f}")
    assert not np.isnan(density).any()
    assert (np.abs(density.astype(np.float64) - want) <= V.tol(N, want)).all(), (case.name, who, err)
    background = ~exp.ref.covered
    assert (density[background] == np.float32(2.0 * case.extent)).all(), (case.name, who)
    assert (material[background] == 0).all()
    check = exp.check_material
    assert (~check).sum() <= V.LEFT_OUT_SHARE * check.size
    assert np.array_equal(material[check], exp.ref.material[check]), (case.name, who)
    assert np.array_equal(material == 1, density <= 0)
    return err


def check_ill(case: V.Case, density, material, who: str):
    """What holds for any input: no NaN, nothing below the shell's floor, a distance is only ever over-estimated where well-conditioned
    triangles alone reach, material = (density <= 0)."""
    N = V.grid(case.resolution, case.extent)[0]
    exp = V.expected(case)
    want = exp.ref.density
    assert exp.ref.ambiguous == 0
    assert not np.isnan(density).any(), (case.name, who)
    t = V.tol(N, want)
    assert (density >= -0.5 - V.tol(N, 0.5)).all(), (case.name, who, float(density.min()))
    w = exp.well_only
    print(f"voxelize_reference: {case.name:28s} {who:6s} worst scaled error {V.scaled_error(N, density[w], want[w]):.3f} on the {int(w.sum())} "
          f"voxels of well-conditioned triangles")
    assert (density[w] >= want[w] - t[w]).all(), (case.name, who)
    assert (density[~exp.ref.covered & w] == np.float32(2.0 * case.extent)).all()
    assert np.array_equal(material == 1, density <= 0)


@pytest.mark.parametrize("name", list(WELL))
def test_cpu_converter_matches_the_reference_on_the_whole_grid(name, capfd):
    case = WELL[name]()
    vol, skipped = cpu_twin(case, capfd)
    assert skipped == case.skipped == 0
    exp = V.expected(case)
    check_well(case, vol.density, vol.material_id, "cpu")
    N = vol.N
    if name.startswith("outside_far"):
        assert not exp.ref.covered.any() and (vol.density == np.float32(2.0 * case.extent)).all() and not vol.material_id.any()
    if name.startswith("outside_near"):
        solid = np.argwhere(vol.material_id == 1)
        assert len(solid) > 0 and (solid[:, 0] == N - 1).all()   # a single layer: the face x = N - 1
    if name.startswith("small_extent"):
        # the background, 1, lies below what the triangles alone would leave in the far part of their boxes, and wins there
        inside = exp.ref.covered & (exp.ref.density == 2.0 * case.extent)
        assert inside.sum() > 1000 and (vol.density[inside] == np.float32(1.0)).all() and (vol.density <= 1.0).all()


def test_the_soups_hold_the_kinds_they_are_built_for():
    """From the reference alone: whole-grid boxes, face-crossing triangles, one-voxel-thin clipped boxes, empty boxes."""
    seen = np.zeros(5, int)
    for res, n, span in soups(SOUP_RESOLUTIONS):
        case = V.clipped_soup(res, n, span)
        have = [k.any() for k in V.kinds(case.triangles(), res, case.extent)]
        want = V.required_kinds(res, span)
        assert all(have[j + 1] for j in range(3) if want[j]), (case.name, have, want)
        seen += have
    assert (seen >= 5).all(), seen
    assert V.required_kinds(4, 0.15) == (True, True, True) and V.required_kinds(3, 1.4) == (True, True, True)


ILL = {f"ill_{seed}_res{res}": (lambda seed=seed, res=res: V.ill_conditioned(seed, res)) for seed in ILL_SEEDS for res in ILL_RESOLUTIONS}
ILL["damaged_res5"] = V.damaged_vertices


@pytest.mark.parametrize("name", list(ILL))
def test_cpu_converter_on_ill_conditioned_and_damaged_input(name, capfd):
    case = ILL[name]()
    vol, skipped = cpu_twin(case, capfd)
    assert skipped == case.skipped
    if name.startswith("damaged"):
        assert case.skipped == 6 and (vol.material_id == 1).sum() > 100  # the good mesh is there
    check_ill(case, vol.density, vol.material_id, "cpu")


def test_reference_rounds_half_away_from_zero_and_counts_ambiguous_edges():
    assert list(V.round_half_away([0.5, 1.5, 2.5, -0.5, -1.5, 2.4999, -2.5001])) == [1, 2, 3, -1, -2, 2, -3]
    N, cell, thr = V.grid(4, 50.0)
    # a triangle whose upper x edge lands exactly on a tie: hi_raw = 9.5
    x = 9.5 * cell - 50.0 - thr
    tri = np.array([[[x - 20, 0, 0], [x, 10, 0], [x - 5, 0, 12]]])
    assert V.boxes(tri, 4, 50.0)[2] == 1
    tri[0, 1, 0] += 0.01 * cell
    assert V.boxes(tri, 4, 50.0)[2] == 0
    # beyond the clip a tie changes nothing: not ambiguous
    tri = np.array([[[0, 0, 0], [10, 10, 0], [(N + 1.5) * cell - 50.0 - thr, 0, 12]]])
    assert V.boxes(tri, 4, 50.0)[2] == 0


def test_reference_at_equals_the_whole_grid():
    case = V.clipped_soup(4, 40, 1.4)
    full = V.expected(case).ref
    at = np.random.RandomState(1).randint(0, 17, (500, 3))
    part = V.reference(case.triangles(), 4, case.extent, at)
    assert np.array_equal(part.density, full.density[at[:, 0], at[:, 2], at[:, 1]])
    assert np.array_equal(part.covered, full.covered[at[:, 0], at[:, 2], at[:, 1]])
