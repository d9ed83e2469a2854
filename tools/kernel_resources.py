#!/usr/bin/env python3
"""Per-kernel register / LDS / scratch use from the -save-temps ISA of the HIP build (amdhsa.kernels metadata).
Usage: python tools/kernel_resources.py [translation unit: vrt_kernels, vrt_volume, vrt_brush, ...] [name filter]
The listing is found and read by tests/isa_listing.py ($VRT_BUILD_TMP, default build/hip)."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import isa_listing  # noqa: E402

unit = sys.argv[1] if len(sys.argv) > 1 else "vrt_kernels"
flt = sys.argv[2] if len(sys.argv) > 2 else ("march" if unit == "vrt_kernels" else "")
for name, f in isa_listing.kernels(unit).items():
    if flt not in name:
        continue
    try:
        name = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", name], capture_output=True, text=True).stdout.strip() or name
    except Exception:
        pass
    v = f.get("vgpr_count", 0)
    print(f"{name[:70]:70s} vgpr {v:4d} (waves/SIMD {min(8, 512 // max(v, 1))})  sgpr {f.get('sgpr_count', 0):4d}  lds {f.get('group_segment_fixed_size', 0):6d}  "
          f"scratch {f.get('private_segment_fixed_size', 0):4d}  spills s{f.get('sgpr_spill_count', 0)} v{f.get('vgpr_spill_count', 0)}")
