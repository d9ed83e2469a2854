"""vrt_volume_components at resolutions 0, 1 and 2 (N = 2, 3, 5: one brick, a single partly filled 8^3 tile) in both formats, with and
without the empty-space tables, and on 257^3 = 2^24 + 197 377 samples: the first grid on which the capped grid-stride loops of the merge,
flatten, roots, mark and apply kernels run a second time and the statistics kernel's lanes meet several components each.  The small
grids go against the numpy reference (tests/components_ref.py), the large one against the host C++ build, so that it stays within a
few seconds.  513^3 reaches no further path of these kernels and its host pass alone takes longer than that: it is left out.
Tolerance 0."""
import functools

import numpy as np
import pytest

import components_ref as CR
import extreme_cases as X
import fill_ref as F
import volume_ref as R
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx
from test_volume_components import record_of
from test_volume_components_gpu import call_and_check
from test_volume_fill_gpu import EDITED, FULL, assert_same_buffers, buffers, upload_field
from test_volume_fill_gpu import _fresh_slots  # noqa: F401 -- the autouse fixture: both slots start unused and are freed after
from test_volume_ops_extremes_gpu import big_volume, same_dense

pytestmark = pytest.mark.gpu


def corners_field(N: int) -> np.ndarray:
    """A component in every corner: single solid samples (N = 2: the four corners of even parity, which touch only over diagonals),
    passable samples at 0.25."""
    x, z, y = np.indices((N,) * 3)
    corner = np.isin(x, (0, N - 1)) & np.isin(y, (0, N - 1)) & np.isin(z, (0, N - 1))
    if N == 2:
        corner &= (x + y + z) % 2 == 0
    return np.where(corner, np.float32(-1.0), np.float32(0.25)).astype(np.float32)


def small_records(N: int, corners: bool):
    out = [dict(op=CR.REPORT), dict(op=CR.KEEP_LARGEST, gap=0.5, material_id=0), dict(op=CR.REMOVE_SMALL, gap=0.5, min_samples=2),
           dict(op=CR.REMOVE_SMALL, gap=0.125, material_id=200, min_samples=N ** 3 + 1)]
    if corners:
        out += [dict(op=CR.KEEP_SEED, gap=0.5, seed=(N - 1, N - 1, N - 1)), dict(op=CR.REMOVE_SEED, gap=0.5, material_id=3, seed=(0, 0, 0))]
    return out


@pytest.mark.parametrize("fmt", X.FORMATS)
@pytest.mark.parametrize("N", X.SMALL)
def test_components_on_the_smallest_grids(renderer, N, fmt):
    written = 0
    d = corners_field(N)
    fields = {"corners": (R.dense_field(d, fmt), F.hand_made_material(d)), "random": X.small_field(N, fmt)}
    for name, (stored, material) in fields.items():
        for kw in small_records(N, name == "corners"):
            want_d, want_m, want = CR.components(stored, material, fmt, list_capacity=20, **kw)
            if name == "corners" and kw["op"] == CR.REPORT:
                assert want["components"] == (4 if N == 2 else 8) and all(c["samples"] == 1 for c in want["list"])
            for table in (True, False):
                got = call_and_check(renderer, X.volume(N, fmt, table), fmt, stored, material, kw, want_d, want_m, want,
                                     f"N {N}, format {fmt}, tables {table}, {name}, {kw}")
                written += got["written"]
    assert written > 0


@functools.lru_cache(maxsize=None)
def specks_257():
    return X.read_only(*CR.specks_field(257))


@functools.lru_cache(maxsize=None)
def specks_257_case(fmt):
    """The stored field, and what the host C++ build makes of it with REMOVE_SMALL."""
    d, m = specks_257()
    stored = R.dense_field(d, fmt)
    vol = big_volume(257, fmt)
    vol.density, vol.material_id = stored.copy(), np.array(m)
    kw = dict(op=CR.REMOVE_SMALL, gap=0.5, material_id=0, min_samples=1000)
    want = vx.components_host(vol, record_of(kw), texel16=fmt == R.TEXEL16, list_capacity=8)
    return kw, X.read_only(stored), m, X.read_only(vol.density), X.read_only(vol.material_id), want


@pytest.mark.parametrize("fmt", X.FORMATS)
def test_remove_small_at_257(renderer, fmt):
    N = 257
    kw, stored, material, want_d, want_m, want = specks_257_case(fmt)
    # the conditions, from the host build alone: one large component stays, a few hundred go, on both sides of lane 2^24
    assert want["components"] > 200 and want["removed"] == want["components"] - 1 and want["list"][0]["samples"] > 800000
    assert want["written"] > want["removed_samples"] > 400  # halo samples among the written
    below, beyond = X.split_by_cap(want_d.view(np.uint32) != stored.view(np.uint32))
    assert below > 0 and beyond > 0, (below, beyond)
    vol = big_volume(N, fmt)
    what = f"257^3 specks, format {fmt}"
    upload_field(renderer, EDITED, vol, fmt, stored, material)
    report = renderer.components(EDITED, record_of(dict(op=CR.REPORT)), None, 8)
    assert report["components"] == want["components"] and report["solid"] == want["solid"] and report["written"] == 0
    assert [dict(c, removed=0) for c in want["list"]] == report["list"]
    got = renderer.components(EDITED, record_of(kw), None, 8)
    print(f"{what}: { {k: got[k] for k in got if k != 'list'} }")
    assert got == want, (got, want)
    have = buffers(renderer, EDITED)
    same_dense(have, want_d, want_m, what)
    upload_field(renderer, FULL, vol, fmt, want_d, want_m)
    assert_same_buffers(have, buffers(renderer, FULL), what + " against a full upload")
    again = renderer.components(EDITED, record_of(kw), None, 8)
    assert again["written"] == 0 and again["components"] == 1, again
    assert_same_buffers(buffers(renderer, EDITED), have, what + " after a second call")
