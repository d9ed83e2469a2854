#!/usr/bin/env python3
"""The C++ adaptor's headers against the reference's own interface declarations, for a machine that has a
checkout of the reference.

The drop-in boundary on the C++ side is `VRenderer` (Renderer/Public/Renderer.h:44-60) and `VTextureFactory`
(Renderer/Public/TextureFactory.h:32-41): a class that overrides this build's csrc/host/HostRenderer.h must override the reference's
header too, so the virtuals' names AND parameter types have to be the same.  The reference's headers are parsed as TEXT (no compile:
they pull in boost / Eigen).  This build's side alone is checked through the library by tests/test_boundary_interface.py.

Usage: python tools/check_reference_interface.py <reference checkout>/VolumetricRaytracer/VolumetricRaytracer/Renderer/Public
Prints one line per check and exits non-zero if any fails."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "volumetricraytracer_amd", "csrc", "host")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _class_body(text, name):
    m = re.search(r"class\s+" + name + r"\b[^;{]*\{", text)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def _members(body):
    """[(name, (parameter types...), kind 'virtual' | 'static' | '', is_override, is_pure)] of the member functions declared in a class body."""
    out = []
    for m in re.finditer(r"([\w:<>\s\*&]+?)\s+(\w+)\s*\(([^()]*)\)\s*(const)?\s*(override)?\s*(=\s*0)?\s*(;|\{)", body):
        ret, name, params = m.group(1).split(), m.group(2), m.group(3)
        kind = "virtual" if "virtual" in ret else "static" if "static" in ret else ""
        if name in ("VRenderer", "if", "for", "while", "return"):
            continue
        types = []
        for prm in (x.strip() for x in params.split(",") if x.strip()):
            prm = re.sub(r"\s+", " ", prm)
            prm = re.sub(r"\s*\b\w+$", "", prm) if re.search(r"[\w>&\*]\s+\w+$", prm) else prm  # drop the parameter's name
            types.append(prm.replace(" &", "&").replace(" *", "*"))
        out.append((name, tuple(types), kind, m.group(5) is not None, m.group(6) is not None))
    return out


def _signatures(body):
    return {(n, t, k) for n, t, k, _, _ in _members(body)}


def _read(path):
    with open(path, encoding="latin-1") as f:
        return _strip_comments(f.read())


def vrenderer_virtuals_are_the_reference_s(ref_dir):
    ref = _signatures(_class_body(_read(os.path.join(ref_dir, "Renderer.h")), "VRenderer"))
    own = _signatures(_class_body(_read(os.path.join(HOST, "HostRenderer.h")), "VRenderer"))
    ref_virtual = {(n, t) for n, t, k in ref if k == "virtual"}
    own_virtual = {(n, t) for n, t, k in own if k == "virtual"}
    assert ("InitializeTexture", ("VObjectPtr<VTexture>",)) in ref_virtual and ("UploadToGPU", ("VObjectPtr<VTexture>",)) in ref_virtual
    assert ref_virtual == own_virtual, (sorted(ref_virtual ^ own_virtual))
    assert {(n, t) for n, t, k in ref if k == ""} >= {("SetRendererMode", ("const EVRenderMode&",))}
    assert ("SetRendererMode", ("const EVRenderMode&",), "") in own
    # the render modes carry the reference's numeric values
    modes = lambda text: re.findall(r"(\w+)\s*=\s*(\d+)", re.search(r"enum class EVRenderMode\s*\{(.*?)\}", text, re.S).group(1))  # noqa: E731
    assert modes(_read(os.path.join(ref_dir, "Renderer.h"))) == modes(_read(os.path.join(HOST, "HostRenderer.h")))


def texture_factory_statics_are_the_reference_s(ref_dir):
    ref = _signatures(_class_body(_read(os.path.join(ref_dir, "TextureFactory.h")), "VTextureFactory"))
    own = _signatures(_class_body(_read(os.path.join(HOST, "HostRenderer.h")), "VTextureFactory"))
    assert len(ref) == 5 and all(k == "static" for _, _, k in ref)
    assert ref == own, sorted(ref ^ own)
    assert ("LoadTextureCubeFromFile", ("std::weak_ptr<VRenderer>", "const std::wstring&"), "static") in own


def hip_renderer_overrides_every_pure_virtual(ref_dir):
    """VHipRenderer must be instantiable against the reference's header: every pure virtual of VRenderer has an `override` with the
    same parameter types in HipRenderer.h."""
    pure = {(n, t) for n, t, k, _, is_pure in _members(_class_body(_read(os.path.join(ref_dir, "Renderer.h")), "VRenderer")) if is_pure}
    assert len(pure) == 7 and ("ResizeRenderOutput", ("unsigned int", "unsigned int")) in pure
    overrides = {(n, t) for n, t, _, is_override, _ in _members(_class_body(_read(os.path.join(HOST, "HipRenderer.h")), "VHipRenderer")) if is_override}
    assert pure <= overrides, sorted(pure - overrides)


def main(ref_dir: str) -> int:
    failed = 0
    for check in (vrenderer_virtuals_are_the_reference_s, texture_factory_statics_are_the_reference_s, hip_renderer_overrides_every_pure_virtual):
        try:
            check(ref_dir)
            print(f"ok    {check.__name__}")
        except AssertionError as e:
            failed += 1
            print(f"FAIL  {check.__name__}: {e}")
    return 1 if failed else 0


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit(__doc__)
    raise SystemExit(main(sys.argv[1]))
