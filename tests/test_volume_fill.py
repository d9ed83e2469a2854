"""Enclosed-cavity fill on the host (VVolumeConverter::FillEnclosed through libvrt_host.so, `voxelizer --solid`) against the numpy
reference of vrt_volume_fill_enclosed's contract (tests/fill_ref.py): tolerance 0 on density bits and material bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fill_ref as F
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi, vox_io
from volumetricraytracer_amd import voxelizer as vx
from volumetricraytracer_amd import workloads as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXELIZER = os.path.join(ROOT, "volumetricraytracer_amd", "lib", "voxelizer")

# voxelized_torus(r): enclosed samples and their box by the reference alone.  The torus lies in the xy plane, so the cavity is thin
# along z: in the density array's own axis order [x, z, y] the boxes read [3, 8, 3]..[13, 8, 13] and [5, 14, 5]..[27, 18, 27]; here
# they are (x, y, z), as vrt_fill_result reports them.
TORUS = {4: (52, (3, 3, 8), (13, 13, 8)), 5: (1136, (5, 5, 14), (27, 27, 18))}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def host_against_reference(vol, wall, material, what):
    """The host fill of `vol` (in place) against fill_ref on the same field; returns the reference's info."""
    before_d, before_m = np.array(vol.density, np.float32), np.array(vol.material_id, np.uint8)
    want_d, want_m, info = F.fill(before_d, before_m, R.F32, wall, material)
    got = vx.fill_enclosed_host(vol, wall, material)
    print(f"{what}: filled {got['filled']} (reference {info['filled']}), box {got['lo']}..{got['hi']}, {info['sweeps']} dilation sweeps")
    assert got["filled"] == info["filled"], what
    if info["filled"]:
        assert got["lo"] == info["lo"] and got["hi"] == info["hi"], what
    else:
        assert all(l > h for l, h in zip(got["lo"], got["hi"])), what
    assert same_bits(vol.density, want_d), what
    assert np.array_equal(vol.material_id, want_m), what
    return info


@pytest.mark.parametrize("res", sorted(TORUS))
def test_host_fill_of_a_voxelized_torus_equals_the_reference(res):
    vol = scenes.voxelized_torus(res)
    shell = np.array(vol.density, np.float32)
    info = host_against_reference(vol, 1.0, 1, f"voxelized_torus({res})")
    filled, lo, hi = TORUS[res]
    assert (info["filled"], info["lo"], info["hi"]) == (filled, lo, hi)
    # only samples that were positive changed, all of them to -(d + 1); the outer surface is the shell's
    changed = vol.density.view(np.uint32) != shell.view(np.uint32)
    assert int(changed.sum()) == filled and (shell[changed] > 0).all()
    assert same_bits(vol.density[changed], -(shell[changed] + np.float32(1.0)))
    assert (vol.material_id[changed] == 1).all()


def test_a_torus_without_a_cavity_fills_nothing():
    vol = scenes.voxelized_torus(3)
    shell = vol.density.copy()
    info = host_against_reference(vol, 1.0, 1, "voxelized_torus(3)")
    assert info["filled"] == 0 and same_bits(vol.density, shell)


@pytest.mark.parametrize("name", sorted(F.hand_made_fields()))
def test_host_fill_of_the_hand_made_fields_equals_the_reference(name):
    d, wall, material, filled, lo, hi = F.hand_made_fields()[name]
    vol = v.VVoxelVolume(5, 100.0)
    vol.density, vol.material_id = d.copy(), F.hand_made_material(d)
    info = host_against_reference(vol, wall, material, name)
    assert info["filled"] == filled, name
    if filled:
        assert (info["lo"], info["hi"]) == (lo, hi), name
    walls = ~F.passable(d)
    assert np.array_equal(vol.density.view(np.uint32)[walls], d.view(np.uint32)[walls])  # walls, NaN and -0.0 among them, keep their bits
    if name == "channel":
        assert same_bits(vol.density[:, 5, :], d[:, 5, :])  # the whole channel stays as it was
    if name == "wall 0, ids untouched":
        written = vol.density.view(np.uint32) != d.view(np.uint32)
        assert same_bits(vol.density[written], -d[written]) and np.array_equal(vol.material_id, F.hand_made_material(d))


def test_reference_properties():
    """A second application fills nothing; neither does a field without a wall or without a passable sample."""
    for fmt in (R.F32, R.TEXEL16):
        for res in (4, 5):
            vol = scenes.voxelized_torus(res)
            stored = R.dense_field(np.array(vol.density, np.float32), fmt)
            mat = np.array(vol.material_id, np.uint8)
            once_d, once_m, first = F.fill(stored, mat, fmt, 1.0, 1)
            # (a texel below one quantum, 0 < d < 0.01, stores 0 and is a wall: the 16-bit field encloses a few samples fewer)
            assert first["filled"] == TORUS[res][0] if fmt == R.F32 else 0 < first["filled"] <= TORUS[res][0]
            twice_d, twice_m, second = F.fill(once_d, once_m, fmt, 1.0, 1)
            assert second["filled"] == 0 and all(l > h for l, h in zip(second["lo"], second["hi"]))
            assert same_bits(twice_d, once_d) and np.array_equal(twice_m, once_m)
        for value in (2.5, -2.5):
            flat = R.dense_field(np.full((17,) * 3, value, np.float32), fmt)
            out, _, info = F.fill(flat, np.zeros(flat.shape, np.uint8), fmt, 1.0, 1)
            assert info["filled"] == 0 and same_bits(out, flat)


def test_host_fill_refuses_bad_arguments():
    vol = v.VVoxelVolume(3, 100.0)
    for wall, material in ((-1.0, 1), (float("nan"), 1), (float("inf"), 1), (1.0, 256), (1.0, -2)):
        with pytest.raises(RuntimeError):
            vx.fill_enclosed_host(vol, wall, material)


def test_voxelizer_solid_writes_the_host_fill_of_the_plain_conversion(tmp_path):
    pos, nrm, idx = vx.torus_mesh(0.55, 0.22, 128, 64)
    gltf = str(tmp_path / "torus.gltf")
    vx.write_gltf(gltf, [("torus_5", pos, nrm, idx, None)], [{"name": "Torus", "mesh": 0}])
    plain, solid = str(tmp_path / "plain.vox"), str(tmp_path / "solid.vox")
    for out, extra in ((plain, []), (solid, ["--solid"])):
        r = subprocess.run([VOXELIZER] + extra + ["--out", out, gltf], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert ("voxelizer, solid" in r.stdout) == bool(extra)
    sc = vox_io.load_scene(plain)
    vol = sc.volumes()[0]
    got = vx.fill_enclosed_host(vol, 1.0, 1)
    assert got["filled"] == TORUS[5][0]
    want = vox_io.load_scene(solid).volumes()[0]
    assert same_bits(want.density, vol.density) and np.array_equal(want.material_id, vol.material_id)
    # and as files: the plain file with its block of VVoxel records replaced by the host-filled ones is the tool's solid file
    raw = open(plain, "rb").read()
    before = vox_io.load_scene(plain).volumes()[0].voxel_records().tobytes()
    at = raw.find(before)
    assert at > 0 and raw.find(before, at + 1) < 0
    assert raw[:at] + vol.voxel_records().tobytes() + raw[at + len(before):] == open(solid, "rb").read()
    assert raw != open(solid, "rb").read()


def test_ctypes_declaration_of_the_fill():
    assert C.sizeof(_abi.vrt_fill_result) == 40
    assert "vrt_volume_fill_enclosed" in _abi.SYMBOLS
