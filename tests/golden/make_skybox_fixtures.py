"""Generates tests/golden/skybox/{XP,XM,YP,YM,ZP,ZM}.png from the reference's sky box faces (data files,
Resources/Skybox/*.png, MIT licence): every chunk is kept as it is (IHDR, iCCP, pHYs, the image data split over several IDAT
chunks, IEND) and so is every filtered scanline with its filter type; only the zlib stream of the image data is re-deflated at
level 9 (the six faces: 2.6 MB -> 2.0 MB).  Decoded, each face is the reference's pixel for pixel.

Run:  python tests/golden/make_skybox_fixtures.py <reference checkout>/VolumetricRaytracer/VolumetricRaytracer/Resources/Skybox
"""
import os
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
FACES = ("XP", "XM", "YP", "YM", "ZP", "ZM")
IDAT_BYTES = 8192


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def recompress(png: bytes) -> bytes:
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, idat, i = [png[:8]], b"", 8
    while i < len(png):
        n, kind = struct.unpack(">I4s", png[i:i + 8])
        data = png[i + 8:i + 8 + n]
        i += 12 + n
        if kind == b"IDAT":
            idat += data
            continue
        if kind == b"IEND":
            z = zlib.compress(zlib.decompress(idat), 9)
            out += [_chunk(b"IDAT", z[k:k + IDAT_BYTES]) for k in range(0, len(z), IDAT_BYTES)]
        out.append(_chunk(kind, data))
    return b"".join(out)


def main(skybox_dir: str) -> None:
    os.makedirs(os.path.join(HERE, "skybox"), exist_ok=True)
    for face in FACES:
        with open(os.path.join(skybox_dir, face + ".png"), "rb") as f:
            png = recompress(f.read())
        with open(os.path.join(HERE, "skybox", face + ".png"), "wb") as f:
            f.write(png)


if __name__ == "__main__":
    main(sys.argv[1])
