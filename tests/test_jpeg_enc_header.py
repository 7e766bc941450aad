"""fid_jpeg_enc_header (host code, no device): the bytes in front of the entropy-coded data must be those of the files
libjpeg-turbo wrote (tests/golden/jpeg_enc_cases.npz) -- one and three components, the three samplings, quality 1, 50, 80 and
100 -- and the call must refuse what the header documents."""
import ctypes as C
import os

import numpy as np

from fiducials_amd import _lib
from fiducials_amd import jpeg as fj

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc_cases.npz")
MONO = 3


def test_header_equals_the_golden_files_leading_bytes():
    gold = np.load(GOLD)
    seen = set()
    for k, w, h, mode, q, _ in gold["cases"].tolist():
        data = gold[f"jpg_{k}"].tobytes()
        nc, sub = (1, 0) if mode == MONO else (3, mode)
        hdr = fj.header(q, sub, w, h, nc)
        assert len(hdr) == (328 if nc == 1 else 623)
        assert data[:len(hdr)] == hdr, (k, w, h, mode, q)
        assert hdr[-10 if nc == 3 else -6:][-3:] == b"\x00\x3f\x00"
        seen.add((mode, q))
    assert {(m, q) for m in range(4) for q in (1, 50, 80, 100)} <= seen


def test_header_is_the_restatements():
    import jpeg_encode_restatement as R

    for nc, sub in ((1, 0), (3, 0), (3, 1), (3, 2)):
        for q in (1, 25, 49, 50, 51, 99, 100):
            assert fj.header(q, sub, 1920, 1080, nc) == R.header(q, sub, 1920, 1080, nc)
    assert fj.header(80, 2, 65535, 1, 3) == R.header(80, 2, 65535, 1, 3)


def test_header_refusals():
    L = _lib.load()
    buf = np.zeros(1024, np.uint8)
    nb = C.c_int64(-1)

    def call(q=80, sub=2, w=64, h=48, nc=3, out=buf.ctypes.data, cap=1024, n=C.byref(nb)):
        return L.fid_jpeg_enc_header(q, sub, w, h, nc, out, cap, n)

    assert call() == _lib.FID_OK and nb.value == 623
    for kw in ({"q": 0}, {"q": 101}, {"q": -5}, {"sub": -1}, {"sub": 3}, {"nc": 2}, {"nc": 0}, {"nc": 4}, {"w": 0}, {"h": 0}, {"w": 65536}, {"h": 65536},
               {"n": None}):
        assert call(**kw) == _lib.FID_E_INVALID_ARG, kw
    nb.value = -1
    assert call(cap=622) == _lib.FID_E_CAPACITY and nb.value == 623  # (the size needed is reported)
    assert call(out=None) == _lib.FID_E_CAPACITY
    assert call(nc=1, cap=328) == _lib.FID_OK and nb.value == 328
    assert call(nc=1, cap=327) == _lib.FID_E_CAPACITY
