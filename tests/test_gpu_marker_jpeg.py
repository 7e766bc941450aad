"""The overlay chain that ends in a file: fid_jpeg_decode(BGR8) -> fid_detect_device -> fid_jpeg_marker_jpeg.  The file must be,
byte for byte, libjpeg-turbo's encoding (Pillow, quality 80, 4:2:0: the encoder's defaults) of the raw marker image
fid_jpeg_marker_image returns for the same frame -- the image that then never has to cross to the host -- and it must decode through
the device decoder to what the oracle decodes it to."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import jpeg_encode_restatement as R
from fiducials_amd import _lib
from fiducials_amd import jpeg as fj
from fiducials_amd._lib import FidError, FidMarker

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tinted(gray, seed):
    rng = np.random.default_rng(seed)
    g = gray.astype(np.int64)
    b = np.clip(g * 0.85 + 20 + rng.integers(-4, 5, g.shape), 0, 255)
    r = np.clip(g * 1.1 - 8 + rng.integers(-4, 5, g.shape), 0, 255)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)  # (RGB, as Pillow takes it)


def marker_image(dec, markers, n, w, h):
    out = np.zeros((h, w, 3), np.uint8)
    rc = _lib.load().fid_jpeg_marker_image(dec._ctx, 0, _lib.ENC["bgr8"], markers, n, 0, out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("name", ["tag_01", "blank"])
def test_marker_jpeg_is_pillows_file_of_the_marker_image(name):
    Image = pytest.importorskip("PIL.Image")
    from fiducials_amd.detector import ArucoDetector
    from oracle import jpeg as oj

    if name == "tag_01":
        rgb = tinted(np.load(os.path.join(GOLD, "tag_01.npz"))["gray"], 1)
    else:
        yy, xx = np.mgrid[0:480, 0:640]
        rgb = np.stack([(xx // 3) % 256, (yy // 2) % 256, np.full_like(xx, 128)], axis=-1).astype(np.uint8)  # smooth: no markers
    h, w = rgb.shape[:2]
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=90, subsampling=2)
    dec = fj.JpegDecoder(max_width=w, max_height=h)
    det = ArucoDetector(7, max_width=w, max_height=h)  # (the dictionary of aruco_images.test)
    enc = fj.JpegEncoder(max_width=w, max_height=h)
    dec.decode(b.getvalue(), "bgr8", to_host=False)
    ptr, dw, dh, stride, fstride = dec.device_ptr()
    L = _lib.load()
    mk = (FidMarker * 64)()
    n = C.c_int32()
    assert L.fid_detect_device(det._ctx, C.c_void_p(ptr), 1, dw, dh, stride, fstride, _lib.ENC["bgr8"], mk, 64, C.byref(n)) == 0
    assert n.value == (1 if name == "tag_01" else 0)
    raw = marker_image(dec, mk, n.value, w, h)
    if n.value:
        assert (raw.reshape(-1, 3) == (0, 255, 0)).all(axis=1).sum() > 100  # the outline is on it
    out = np.zeros(enc.max_file_bytes, np.uint8)
    nb = C.c_int64()
    for _ in range(2):
        assert L.fid_jpeg_marker_jpeg(dec._ctx, 0, _lib.ENC["bgr8"], mk, n.value, 0, enc._ctx, out.ctypes.data, out.nbytes, C.byref(nb)) == 0
        got = out[:nb.value].tobytes()
        want = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(raw[..., ::-1])).save(want, "JPEG", quality=80, subsampling=2)
        assert got == want.getvalue()
    assert got == R.encode(np.ascontiguousarray(raw[..., ::-1]), 80, 2)
    assert len(got) * 10 < raw.nbytes  # what crosses the link
    # the Python wrapper gives the same file, and the file decodes on the device to what the oracle decodes it to
    corners = np.array([list(mk[i].corners) for i in range(n.value)], np.float32).reshape(-1, 4, 2)
    assert dec.marker_jpeg(0, "bgr8", corners, enc) == got
    back = fj.JpegDecoder(max_width=w, max_height=h)
    assert np.array_equal(back.decode(got, "bgr8"), oj.decode(got))
    # refusals: a room that is too small names the size; the other base image; an encoder that is too small
    with pytest.raises(FidError) as e:
        small = fj.JpegEncoder(max_width=w, max_height=h, max_file_bytes=len(got) - 1)
        dec.marker_jpeg(0, "bgr8", corners, small)
    assert e.value.status == _lib.FID_E_CAPACITY and str(len(got)) in str(e.value)
    assert L.fid_jpeg_marker_jpeg(dec._ctx, 0, _lib.ENC["bgr8"], mk, n.value, 0, enc._ctx, out.ctypes.data, len(got) - 1, C.byref(nb)) == _lib.FID_E_CAPACITY
    assert L.fid_jpeg_marker_jpeg(dec._ctx, 0, _lib.ENC["mono8"], mk, n.value, 0, enc._ctx, out.ctypes.data, out.nbytes, C.byref(nb)) == _lib.FID_E_INVALID_ARG
    assert L.fid_jpeg_marker_jpeg(dec._ctx, 1, _lib.ENC["bgr8"], mk, n.value, 0, enc._ctx, out.ctypes.data, out.nbytes, C.byref(nb)) == _lib.FID_E_INVALID_ARG
    assert L.fid_jpeg_marker_jpeg(dec._ctx, 0, _lib.ENC["bgr8"], mk, n.value, 0, None, out.ctypes.data, out.nbytes, C.byref(nb)) == _lib.FID_E_INVALID_ARG
    tiny = fj.JpegEncoder(max_width=w - 1, max_height=h)
    assert L.fid_jpeg_marker_jpeg(dec._ctx, 0, _lib.ENC["bgr8"], mk, n.value, 0, tiny._ctx, out.ctypes.data, out.nbytes, C.byref(nb)) == _lib.FID_E_INVALID_ARG
    for o in (dec, det, enc, back, small, tiny):
        o.close()
