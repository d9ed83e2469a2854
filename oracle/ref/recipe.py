"""Builds oracle/_ref/ref_probe: the reference's own C++ (everything in it that needs no Direct3D) linked with our driver,
oracle/ref/probe.cpp.  Run by `make -C oracle ref`, which __graft_entry__.build() calls.

The reference tree is read from VRT_REFERENCE_ROOT (default /root/reference).  Its files are never edited and never enter the
repository: the sources listed in SOURCES are copied to oracle/_ref/src/ (ignored by git), the token rules of RULES are
applied to the copies, and the copies are compiled against the reference's own headers plus the stand-ins of
oracle/ref/shims/.  A rule that matches nothing is an error: it would mean the reference changed under the recipe.

Skip rule: with no reference tree and no oracle/_ref/ref_probe already there, one line is printed and the step succeeds
(a GPU machine has neither and needs neither: its tests read committed fixtures only)."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "_ref")
PROBE = os.path.join(OUT, "ref_probe")
INFO = os.path.join(OUT, "build_info.json")

TREE = "VolumetricRaytracer"  # below the root
INCLUDE_DIRS = ["VolumetricRaytracer/Core/Public", "VolumetricRaytracer/Voxel/Public", "VolumetricRaytracer/Scene/Public", "Voxelizer/Public"]
SOURCES = [
    "VolumetricRaytracer/Core/Private/AABB.cpp",
    "VolumetricRaytracer/Core/Private/Color.cpp",
    "VolumetricRaytracer/Core/Private/Material.cpp",
    "VolumetricRaytracer/Core/Private/MathHelpers (2).cpp",
    "VolumetricRaytracer/Core/Private/Object.cpp",
    "VolumetricRaytracer/Core/Private/Quat.cpp",
    "VolumetricRaytracer/Core/Private/SerializationManager.cpp",
    "VolumetricRaytracer/Core/Private/StringHelpers.cpp",
    "VolumetricRaytracer/Core/Private/TickManager.cpp",
    "VolumetricRaytracer/Core/Private/Vector.cpp",
    "VolumetricRaytracer/Voxel/Private/Octree.cpp",
    "VolumetricRaytracer/Voxel/Private/Voxel.cpp",
    "VolumetricRaytracer/Voxel/Private/VoxelVolume.cpp",
    "VolumetricRaytracer/Scene/Private/Camera.cpp",
    "VolumetricRaytracer/Scene/Private/DensityGenerator.cpp",
    "VolumetricRaytracer/Scene/Private/LevelObject.cpp",
    "VolumetricRaytracer/Scene/Private/Light.cpp",
    "VolumetricRaytracer/Scene/Private/PointLight.cpp",
    "VolumetricRaytracer/Scene/Private/Scene.cpp",
    "VolumetricRaytracer/Scene/Private/SpotLight.cpp",
    "VolumetricRaytracer/Scene/Private/VoxelObject.cpp",
    "Voxelizer/Private/SceneConverter.cpp",
    "Voxelizer/Private/VolumeConverter.cpp",
]
# (file name, token to find, token to put): single tokens, no context.  g++ rejects binding a lambda to a non-const
# reference and constructing a stream from a wide string; MSVC accepts both.
RULES = [
    ("VolumeConverter.cpp", "auto& getPositionAlongRay", "auto getPositionAlongRay"),
    ("VolumeConverter.cpp", "auto& signFunc", "auto signFunc"),
    ("SerializationManager.cpp", "std::ifstream(filePath,", "std::ifstream(std::filesystem::path(filePath),"),
]
CXX = os.environ.get("CXX", "g++")
# -O1 without -march: SSE2 scalar fp32, no contraction possible, the same sums in the same order on every x86-64
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-w", "-fpermissive"]


def main() -> int:
    root = os.path.join(os.environ.get("VRT_REFERENCE_ROOT", "/root/reference"), TREE)
    if not os.path.isdir(root):
        if os.path.exists(PROBE):
            print(f"oracle/ref: no reference tree at {root}; keeping the existing oracle/_ref/ref_probe")
        else:
            print(f"oracle/ref: no reference tree at {root} and no oracle/_ref/ref_probe: step skipped")
        return 0
    own = [os.path.join(HERE, "probe.cpp"), os.path.abspath(__file__)]
    for d, _, names in os.walk(os.path.join(HERE, "shims")):
        own += [os.path.join(d, n) for n in sorted(names)]
    h = hashlib.sha256()
    for p in sorted(own) + [os.path.join(root, s) for s in SOURCES]:
        with open(p, "rb") as f:
            h.update(p.encode() + b"\0" + f.read())
    for d in INCLUDE_DIRS:
        for n in sorted(os.listdir(os.path.join(root, d))):
            p = os.path.join(root, d, n)
            if os.path.isfile(p):
                with open(p, "rb") as f:
                    h.update(f.read())
    stamp = h.hexdigest()
    if os.path.exists(PROBE) and os.path.exists(INFO):
        with open(INFO) as f:
            if json.load(f).get("stamp") == stamp:
                return 0
    src = os.path.join(OUT, "src")
    shutil.rmtree(src, ignore_errors=True)
    os.makedirs(src)
    copies = []
    used = set()
    for s in SOURCES:
        name = os.path.basename(s).replace(" (2)", "")
        with open(os.path.join(root, s), "rb") as f:
            text = f.read()
        for i, (where, find, put) in enumerate(RULES):
            if where == name:
                if find.encode() not in text:
                    print(f"oracle/ref: rule {find!r} matches nothing in {s}: the reference changed, fix the recipe", file=sys.stderr)
                    return 1
                text = text.replace(find.encode(), put.encode())
                used.add(i)
        copies.append(os.path.join(src, name))
        with open(copies[-1], "wb") as f:
            f.write(text)
    if len(used) != len(RULES):
        print("oracle/ref: a rule names a file that is not built", file=sys.stderr)
        return 1
    includes = ["-I" + os.path.join(HERE, "shims")] + ["-I" + os.path.join(root, d) for d in INCLUDE_DIRS]
    base = [CXX] + FLAGS + ["-include", os.path.join(HERE, "shims", "prelude.h")] + includes

    def compile_one(path):
        obj = os.path.join(src, os.path.splitext(os.path.basename(path))[0] + ".o")
        r = subprocess.run(base + ["-c", path, "-o", obj], capture_output=True, text=True)
        return obj, r

    objs = []
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for obj, r in pool.map(compile_one, copies + [os.path.join(HERE, "probe.cpp")]):
            if r.returncode != 0:
                print(r.stderr[-6000:], file=sys.stderr)
                return 1
            objs.append(obj)
    r = subprocess.run([CXX, "-o", PROBE] + objs + ["-pthread"], capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stderr[-6000:], file=sys.stderr)
        return 1
    with open(INFO, "w") as f:
        json.dump({"stamp": stamp, "compiler_line": " ".join([os.path.basename(CXX)] + FLAGS + ["-include shims/prelude.h -Ishims"]),
                   "files": SOURCES, "rules": [list(r) for r in RULES]}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
