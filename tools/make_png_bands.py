#!/usr/bin/env python3
"""tests/golden/<name>.rows_<a>_<b>.png: a band of rows of the reference's PNG test images (aruco_detect/test/test_images), small
enough to commit.  Rows a + 1 .. b - 1 keep the reference file's own filter byte and filtered bytes, exactly as its encoder wrote
them; row a (the row above the band, the one the Up / Average / Paeth filters of the band's first row read) is stored
reconstructed, with filter 0.  IHDR (height b - a), the ancillary chunks and the IDAT chunk size are the original's; only the
deflate layer (zlib's, not the product's) is encoded anew.  Decoded, the band is rows a .. b - 1 of the original image.
Run in the authoring container (needs /root/reference and Pillow)."""
import io
import os
import struct
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/aruco_detect/test/test_images/"
GOLD = os.path.join(ROOT, "tests", "golden")
BANDS = {"tag_01_d7_14cm": (119, 504), "tag_245-246_d7_14cm": (119, 440)}


def chunks(data):
    pos = 8
    while pos < len(data):
        n, t = struct.unpack(">I4s", data[pos:pos + 8])
        yield t, data[pos + 8:pos + 8 + n]
        pos += 12 + n


def chunk(t, body):
    return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body) & 0xFFFFFFFF)


def band(data, a, b):
    cs = list(chunks(data))
    ihdr = dict(cs)[b"IHDR"]
    w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", ihdr)
    assert (depth, ctype, interlace) == (8, 2, 0), (depth, ctype, interlace)  # 8-bit RGB, not interlaced
    stride = 1 + 3 * w
    raw = zlib.decompress(b"".join(body for t, body in cs if t == b"IDAT"))
    assert len(raw) == stride * h
    full = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    rows = b"\0" + full[a].tobytes() + raw[(a + 1) * stride:b * stride]
    z = zlib.compress(rows, 9)
    size = max(len(body) for t, body in cs if t == b"IDAT")
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, b - a, 8, 2, 0, 0, 0))
    out += b"".join(chunk(t, body) for t, body in cs if t not in (b"IHDR", b"IDAT", b"IEND"))
    out += b"".join(chunk(b"IDAT", z[i:i + size]) for i in range(0, len(z), size)) + chunk(b"IEND", b"")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(out)).convert("RGB")), full[a:b])
    return out


def main():
    for name, (a, b) in BANDS.items():
        out = band(open(REF + name + ".png", "rb").read(), a, b)
        path = os.path.join(GOLD, f"{name}.rows_{a}_{b}.png")
        open(path, "wb").write(out)
        print(path, len(out))


if __name__ == "__main__":
    main()
