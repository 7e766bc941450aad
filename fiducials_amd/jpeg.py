"""JPEG ingest on the device -- Python mirror of the `fid_jpeg_*` entry points (include/fid_abi.h): what image_transport's
compressed subscriber + cv::imdecode do in front of FiducialsNode::imageCallback when the node runs with its launch default
`transport:=compressed` (aruco_detect/launch/aruco_detect.launch:6)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FidError

TAP_COEFS, TAP_PLANES = 0, 1


def probe(data: bytes) -> dict:
    """Header parse on the host: size, components, sampling, restart interval, block counts."""
    L = _lib.load()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    info = _lib.FidJpegInfo()
    rc = L.fid_jpeg_probe(C.cast(buf, C.c_void_p), len(data), C.byref(info))
    if rc != _lib.FID_OK:
        raise FidError(rc, L.fid_strerror(rc).decode())
    return {"width": info.width, "height": info.height, "components": info.components, "h_samp": info.h_samp, "v_samp": info.v_samp,
            "restart_interval": info.restart_interval, "blocks_w": list(info.blocks_w), "blocks_h": list(info.blocks_h),
            "scan_bytes": info.scan_bytes}


class JpegDecoder:
    def __init__(self, max_width: int = 1920, max_height: int = 1080, max_batch: int = 1, device: int = 0):
        self._L = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._L.fid_jpeg_create(device, max_width, max_height, max_batch, C.byref(self._ctx))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        self.max_batch = max_batch
        self.max_width, self.max_height = max_width, max_height

    def close(self):
        if self._ctx:
            self._L.fid_jpeg_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _check(self, rc):
        if rc != _lib.FID_OK:
            raise FidError(rc, (self._L.fid_jpeg_last_error(self._ctx) or b"").decode() or self._L.fid_strerror(rc).decode())

    def decode(self, files, encoding: str = "bgr8", to_host: bool = True):
        """files: a bytes object or a list of them (one image size per call).  -> (n, H, W, 3) bgr8 as cv::imdecode returns it,
        or (n, H, W) mono8 = cvtColor(BGR2GRAY) of that; None with to_host=False (the result stays on the device: device_ptr())."""
        single = isinstance(files, (bytes, bytearray, memoryview))
        blobs = [bytes(files)] if single else [f if isinstance(f, bytes) else bytes(f) for f in files]
        n = len(blobs)
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs])  # (the bytes objects themselves: no copy)
        sizes = (C.c_int64 * n)(*[len(b) for b in blobs])
        i = probe(blobs[0])
        bpp = 1 if encoding == "mono8" else 3
        out = np.empty((n, i["height"], i["width"]) + ((3,) if bpp == 3 else ()), np.uint8) if to_host else None
        rc = self._L.fid_jpeg_decode(self._ctx, ptrs, sizes, n, _lib.ENC[encoding], out.ctypes.data if to_host else None,
                                     i["height"] * i["width"] * bpp)
        self._check(rc)
        self._last = (n, i)
        if not to_host:
            return None
        return out[0] if single else out

    def device_ptr(self):
        """-> (device pointer, width, height, stride, frame stride) of the last decode's output"""
        w, h, s, fs = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        p = self._L.fid_jpeg_device_ptr(self._ctx, C.byref(w), C.byref(h), C.byref(s), C.byref(fs))
        return p, w.value, h.value, s.value, fs.value

    def tap(self, which: int, frame: int = 0) -> np.ndarray:
        nb = self._L.fid_jpeg_tap_bytes(self._ctx, which, frame)
        out = np.empty(nb // 2 if which == TAP_COEFS else nb, np.int16 if which == TAP_COEFS else np.uint8)
        self._check(self._L.fid_jpeg_tap_read(self._ctx, which, frame, out.ctypes.data, nb))
        return out

    def last_rounds(self) -> int:
        return int(self._L.fid_jpeg_last_rounds(self._ctx))

    def marker_jpeg(self, frame: int, base: str, markers, encoder: "JpegEncoder", flags: int = 0) -> bytes:
        """The marker image of frame `frame` of the last decode (what fid_jpeg_marker_image returns: the decoded `base` image as
        BGR with the outlines of `markers`, an (n, 4, 2) array of corners) as the JPEG file `encoder` makes of it on the device."""
        q = np.asarray(markers, np.float32).reshape(-1, 8)
        mk = (_lib.FidMarker * max(len(q), 1))()
        for i in range(len(q)):
            mk[i].id = i
            for j in range(8):
                mk[i].corners[j] = float(q[i, j])
        out = np.empty(encoder.max_file_bytes, np.uint8)
        nb = C.c_int64()
        self._check(self._L.fid_jpeg_marker_jpeg(self._ctx, frame, _lib.ENC[base], mk, len(q), flags, encoder._ctx, out.ctypes.data, out.nbytes,
                                                 C.byref(nb)))
        return out[:nb.value].tobytes()


def header(quality: int, subsampling: int, width: int, height: int, components: int) -> bytes:
    """The bytes in front of the entropy-coded data of the file the encoder writes (host code, no device)."""
    L = _lib.load()
    out = np.empty(1024, np.uint8)
    nb = C.c_int64()
    rc = L.fid_jpeg_enc_header(quality, subsampling, width, height, components, out.ctypes.data, out.nbytes, C.byref(nb))
    if rc != _lib.FID_OK:
        raise FidError(rc, L.fid_strerror(rc).decode())
    return out[:nb.value].tobytes()


class JpegEncoder:
    """cv::imencode(".jpg") on the device -- Python mirror of the `fid_jpeg_enc_*` entry points: the file libjpeg(-turbo) writes
    with its defaults at `quality` and chroma `subsampling` (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), byte for byte."""

    def __init__(self, max_width: int = 1920, max_height: int = 1080, max_batch: int = 1, quality: int = 80, subsampling: int = 2, device: int = 0,
                 max_file_bytes: int = 0):
        self._L = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._L.fid_jpeg_enc_create(device, max_width, max_height, max_batch, max_file_bytes, C.byref(self._ctx))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        self.max_width, self.max_height, self.max_batch = max_width, max_height, max_batch
        # (the default of fid_jpeg_enc_create: two bytes a pixel of the MCU-padded frame + 64 KiB + the header)
        self.max_file_bytes = max_file_bytes or ((max_width + 15) // 16 * 16) * ((max_height + 15) // 16 * 16) * 2 + 65536 + 640
        self.set(quality, subsampling)

    def close(self):
        if self._ctx:
            self._L.fid_jpeg_enc_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _check(self, rc):
        if rc != _lib.FID_OK:
            raise FidError(rc, (self._L.fid_jpeg_enc_last_error(self._ctx) or b"").decode() or self._L.fid_strerror(rc).decode())

    def set(self, quality: int, subsampling: int):
        self._check(self._L.fid_jpeg_enc_set(self._ctx, quality, subsampling))
        self.quality, self.subsampling = quality, subsampling

    def _files(self, call, n):
        out = np.empty((n, self.max_file_bytes), np.uint8)
        sizes = (C.c_int64 * n)()
        self._check(call(out.ctypes.data, self.max_file_bytes, sizes))
        return [out[f, :sizes[f]].tobytes() for f in range(n)]

    def encode(self, frames, encoding: str = "bgr8"):
        """frames: (n, H, W) mono8 or (n, H, W, 3) bgr8 / rgb8 (or one frame without the leading axis) -> a list of `bytes`."""
        a = np.ascontiguousarray(frames, np.uint8)
        if a.ndim == (2 if encoding == "mono8" else 3):
            a = a[None]
        n, h, w = a.shape[:3]
        bpp = _lib.ENC_BYTES_PER_PIXEL[encoding]
        return self._files(lambda out, cap, sizes: self._L.fid_jpeg_encode(self._ctx, a.ctypes.data, n, w, h, w * bpp, h * w * bpp, _lib.ENC[encoding], out,
                                                                           cap, sizes), n)

    def encode_device(self, ptr: int, n: int, width: int, height: int, stride: int, frame_stride: int, encoding: str = "bgr8"):
        """n frames in device memory (a torch tensor's data_ptr(), JpegDecoder.device_ptr()) -> a list of `bytes`."""
        return self._files(lambda out, cap, sizes: self._L.fid_jpeg_encode_device(self._ctx, C.c_void_p(ptr), n, width, height, stride, frame_stride,
                                                                                  _lib.ENC[encoding], out, cap, sizes), n)

    def last_ms(self) -> float:
        """device time of the last call's launches (events on the context's stream), ms"""
        return float(self._L.fid_jpeg_enc_last_ms(self._ctx))

    def tap(self, frame: int = 0) -> np.ndarray:
        """int16 quantised coefficients of the last call's frame `frame`, natural order, component after component,
        [blocks_h][blocks_w][64] each (the layout of the decoder's TAP_COEFS)"""
        nb = self._L.fid_jpeg_enc_tap_bytes(self._ctx, frame)
        out = np.empty(nb // 2, np.int16)
        self._check(self._L.fid_jpeg_enc_tap_read(self._ctx, frame, out.ctypes.data, nb))
        return out
