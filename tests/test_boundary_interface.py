"""The C++ adaptor's drop-in boundary: `VTextureFactory`'s five functions and VHipRenderer's base-typed virtuals,
checked through the library (vrh_texture_factory_probe).  The comparison of the adaptor's headers with the reference's own
declarations needs a checkout of the reference: tools/check_reference_interface.py."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_texture_factory_and_base_typed_virtuals_work(tmp_path):
    """This build's side without a GPU: the five factory functions through a renderer that counts InitializeTexture calls, and
    VHipRenderer::InitializeTexture with a base-typed argument."""
    lib_path = os.environ.get("VRT_HOST_LIB") or os.path.join(ROOT, "volumetricraytracer_amd", "lib", "libvrt_host.so")
    if not os.path.exists(lib_path):
        import __graft_entry__

        __graft_entry__.build()
    from volumetricraytracer_amd import _abi

    _abi.load()  # maps the HIP runtime and libvrt_hip.so first (libvrt_host.so's DT_NEEDED)
    lib = C.CDLL(lib_path)
    lib.vrh_texture_factory_probe.restype = C.c_int
    lib.vrh_texture_factory_probe.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.vrh_last_error.restype = C.c_char_p
    # a 5x3 binary PPM and a folder of six 4x4 faces
    img = tmp_path / "t.ppm"
    img.write_bytes(b"P6\n5 3\n255\n" + bytes(range(45)))
    faces = tmp_path / "sky"
    faces.mkdir()
    from volumetricraytracer_amd import vox_io  # noqa: F401  (keeps the package import honest)
    import zlib, struct

    def png(path, w, h):
        raw = b"".join(b"\x00" + bytes([x * 9 % 256, y * 17 % 256, 80, 255] * 1)[0:4] * w for y in range(h) for x in [0])
        def chunk(t, d):
            return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
        path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))

    for f in ("XP", "XM", "YP", "YM", "ZP", "ZM"):
        png(faces / (f + ".png"), 4, 4)
    dims = (C.c_int * 8)()
    rc = lib.vrh_texture_factory_probe(str(img).encode(), str(faces).encode(), dims)
    assert rc == 0, lib.vrh_last_error()
    assert list(dims) == [5, 3, 4, 3, 2, 6, 7, 5]  # five factory calls, five InitializeTexture calls
    assert lib.vrh_texture_factory_probe(str(tmp_path / "missing.png").encode(), b"", dims) == -1
