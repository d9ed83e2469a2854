"""vrt_volume_mask_apply on the host (VVolumeConverter::MaskOps through libvrt_host.so's vrh_mask_apply, which compiles the same
csrc/mask_core.h as the HIP kernels): the byte mask it leaves equals the numpy reference of the contract (tests/mask_ref.py) bit for
bit over tests/mask_cases.py, with equal counts and boxes; one call of n records leaves what n calls of one record leave; every argument
rule refuses; and the two records have the sizes vrt.h states.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extreme_cases as X
import mask_cases as MC
import mask_ref as MK
import session_model as M
import volume_ref as R
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (R.F32, R.TEXEL16)


def records_of(stored, material):
    rec = np.zeros(stored.size, M.VOXEL)
    rec["density"], rec["material"] = stored.reshape(-1), material.reshape(-1)
    return rec


def host_apply(stored, material, fmt, ops, mask=None):
    """vrh_mask_apply on a byte mask (None: zeros): (status, mask as bool [x, z, y], info dict)."""
    N = stored.shape[0]
    voxels = records_of(stored, material)
    out = np.zeros((N, N, N), np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8)
    arr = (_abi.vrt_mask_op * max(1, len(ops)))(*ops)
    info = _abi.vrt_mask_info()
    rc = vx.load_host().vrh_mask_apply(voxels.ctypes.data, N, int(fmt == R.TEXEL16), out.ctypes.data, len(ops), arr, C.byref(info))
    assert set(np.unique(out)) <= {0, 1}
    return rc, out != 0, _abi.mask_info_dict(info)


@pytest.mark.parametrize("N", MC.SIZES)
def test_the_cases_are_what_they_say(N):
    for fmt in FORMATS:
        MC.check_cases_are_what_they_say(N, MC.reference(N, fmt))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", MC.SIZES)
def test_the_host_pass_equals_the_reference(N, fmt):
    stored, material = X.small_field(N, fmt)
    ref = MC.reference(N, fmt)
    for name, ops in MC.cases(N):
        rc, got, info = host_apply(stored, material, fmt, ops)
        assert rc == _abi.VRT_OK, name
        assert np.array_equal(got, ref[name]), (name, int((got != ref[name]).sum()))
        assert info == MK.info(ref[name]), (name, info)


@pytest.mark.parametrize("N", (5, 65))
def test_one_call_of_n_records_is_n_calls_of_one(N):
    stored, material = X.small_field(N, R.F32)
    ops = dict(MC.cases(N))["a sequence"]
    mask = None
    for op in ops:
        rc, mask, _ = host_apply(stored, material, R.F32, [op], mask)
        assert rc == _abi.VRT_OK
    assert np.array_equal(mask, MC.reference(N, R.F32)["a sequence"])


def test_bytes_other_than_0_and_1_protect():
    stored, material = X.small_field(5, R.F32)
    mask = np.zeros((5, 5, 5), np.uint8)
    mask[1, 2, 3], mask[4, 4, 4], mask[0, 0, 0] = 255, 2, 1
    rc, got, info = host_apply(stored, material, R.F32, [], mask)
    assert rc == _abi.VRT_OK and np.array_equal(got, mask != 0) and info == MK.info(mask != 0)


def test_every_argument_rule():
    stored, material = X.small_field(3, R.F32)
    host = vx.load_host()
    for what, ops in MC.refused_records():
        before = np.ones((3, 3, 3), np.uint8)
        rc, got, _ = host_apply(stored, material, R.F32, ops, before)
        assert rc == _abi.VRT_ERR_INVALID, what
        assert got.all(), what  # nothing written
    for ops in MC.accepted_records():
        assert host_apply(stored, material, R.F32, ops)[0] == _abi.VRT_OK, [o.kind for o in ops]
    voxels, mask, one = records_of(stored, material), np.zeros(27, np.uint8), (_abi.vrt_mask_op * 1)(MK.op(MK.ALL, 1))
    assert host.vrh_mask_apply(None, 3, 0, mask.ctypes.data, 1, one, None) == _abi.VRT_ERR_INVALID
    assert host.vrh_mask_apply(voxels.ctypes.data, 3, 0, None, 1, one, None) == _abi.VRT_ERR_INVALID
    assert host.vrh_mask_apply(voxels.ctypes.data, 3, 0, mask.ctypes.data, 1, None, None) == _abi.VRT_ERR_INVALID
    assert host.vrh_mask_apply(voxels.ctypes.data, 3, 0, mask.ctypes.data, -1, one, None) == _abi.VRT_ERR_INVALID
    assert host.vrh_mask_apply(voxels.ctypes.data, 1, 0, mask.ctypes.data, 1, one, None) == _abi.VRT_ERR_INVALID
    assert host.vrh_mask_apply(voxels.ctypes.data, 3, 0, mask.ctypes.data, 1, one, None) == _abi.VRT_OK and mask.all()


def test_the_entry_points_refuse_null_arguments_without_a_device():
    lib = _abi.load()
    one = (_abi.vrt_mask_op * 1)(MK.op(MK.ALL, 1))
    info = _abi.vrt_mask_info()
    byte = (C.c_uint8 * 1)()
    assert lib.vrt_volume_mask_apply(None, 0, 1, one, C.byref(info)) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_mask_upload(None, 0, byte) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_mask_download(None, 0, byte) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_mask_clear(None, 0) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_mask_info(None, 0, C.byref(info)) == _abi.VRT_ERR_INVALID


def test_record_sizes_match_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(vrt_mask_op), sizeof(vrt_mask_info), offsetof(vrt_mask_op, a),'
                    ' offsetof(vrt_mask_op, material), offsetof(vrt_mask_op, reserved_), offsetof(vrt_mask_info, lo),'
                    ' offsetof(vrt_mask_info, restored));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [64, 48]
    assert got == [C.sizeof(_abi.vrt_mask_op), C.sizeof(_abi.vrt_mask_info), _abi.vrt_mask_op.a.offset, _abi.vrt_mask_op.material.offset,
                   _abi.vrt_mask_op.reserved_.offset, _abi.vrt_mask_info.lo.offset, _abi.vrt_mask_info.restored.offset]
