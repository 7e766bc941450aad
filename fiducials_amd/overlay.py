"""The /fiducial_images overlay (aruco_detect.cpp:381-387) on top of the C-ABI: `to_bgr` = cv_bridge::toCvCopy(msg, BGR8),
`draw_detected_markers` = the part of aruco::drawDetectedMarkers that is restated exactly (the four LINE_8 sides of every
marker; include/fid_abi.h says what is not drawn and why).  Host code on both sides: no GPU needed.  `to_bgr_device` and
`draw_detected_markers_device` below do the same, byte for byte, on torch tensors in GPU memory."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FidError, FidMarker

FIRST_CORNER_LINE8 = 1
_BYTES_PER_PIXEL = {"mono8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "mono16": 2, "bgr16": 6, "rgb16": 6, "bgra16": 8, "rgba16": 8,
                    "yuv422": 2, "bayer_rggb8": 1, "bayer_bggr8": 1, "bayer_gbrg8": 1, "bayer_grbg8": 1}


def to_bgr(image: np.ndarray, encoding: str | None = None) -> np.ndarray:
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if encoding is None:
        encoding = "mono8" if img.ndim == 2 else ("bgra8" if img.shape[2] == 4 else "bgr8")
    h, w = img.shape[:2]
    out = np.empty((h, w, 3), dtype=np.uint8)
    rc = _lib.load().fid_to_bgr(img.ctypes.data, w, h, img.strides[0], _lib.ENC[encoding], out.ctypes.data, out.nbytes)
    if rc != _lib.FID_OK:
        raise FidError(rc, "fid_to_bgr")
    return out


def image_to_bgr8(data: np.ndarray, width: int, height: int, step: int, encoding: str, is_bigendian: bool = False) -> np.ndarray:
    """cv_bridge::toCvCopy(msg, "bgr8") of a sensor_msgs/Image given by its fields (data: the message bytes): the five 8-bit
    encodings, mono16 / bgr16 / rgb16 / bgra16 / rgba16 and the four 8-bit Bayer patterns (fid_image_to_bgr8)."""
    # the message BYTES: an ndarray of another dtype (a mono16 frame as uint16) is reinterpreted, never value-converted
    if isinstance(data, np.ndarray):
        buf = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    else:
        buf = np.frombuffer(data, dtype=np.uint8)
    width, height, step = int(width), int(height), int(step)
    bpp = _BYTES_PER_PIXEL.get(encoding)
    if width < 1 or height < 1 or (bpp is not None and step < width * bpp) or buf.size < step * height:
        # (the C side reads step * (height - 1) + a row, the Bayer rows two ahead: a short buffer is refused here, as
        #  FiducialsNode::imageCallback refuses data.size() < step * height)
        raise FidError(_lib.FID_E_INVALID_ARG, f"fid_image_to_bgr8({encoding}): {buf.size} bytes for step {step} x height {height}")
    out = np.empty((height, width, 3), dtype=np.uint8)
    rc = _lib.load().fid_image_to_bgr8(buf.ctypes.data, width, height, step, encoding.encode(), int(bool(is_bigendian)), out.ctypes.data, out.nbytes)
    if rc != _lib.FID_OK:
        raise FidError(rc, f"fid_image_to_bgr8({encoding})")
    return out


def draw_detected_markers(bgr: np.ndarray, corners: np.ndarray, ids: np.ndarray | None = None, flags: int = 0) -> np.ndarray:
    """In place on a (H, W, 3) uint8 BGR image; corners (n, 4, 2) float32.  Returns the image."""
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3 or bgr.strides[2] != 1 or bgr.strides[1] != 3:
        raise ValueError("draw_detected_markers takes a (H, W, 3) uint8 image with packed pixels")
    c = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
    n = len(c)
    mk = (FidMarker * max(n, 1))()
    for i in range(n):
        mk[i].id = int(ids[i]) if ids is not None else 0
        for j in range(8):
            mk[i].corners[j] = float(c[i, j])
    h, w = bgr.shape[:2]
    rc = _lib.load().fid_draw_detected_markers(bgr.ctypes.data, w, h, bgr.strides[0], mk, n, flags)
    if rc != _lib.FID_OK:
        raise FidError(rc, "fid_draw_detected_markers")
    return bgr


# ---- the same overlay on frames in device memory (torch uint8 tensors on the GPU): fid_to_bgr_device / fid_draw_detected_markers_device.
# The bytes are those of to_bgr / draw_detected_markers, frame by frame.  The work queued on the tensors' current stream is waited
# for first (the library reads frames that are complete when it is called and returns when it is done).
_MARKER = np.dtype([("id", "<i4"), ("corners", "<f4", 8)])  # fid_marker
_ENC_OF_CHANNELS = {1: "mono8", 3: "bgr8", 4: "bgra8"}


def _frames(t, name: str):
    """a [N, H, W, C] or [H, W, C] uint8 cuda tensor -> (batch tensor, single, N, H, W, C, row stride, frame stride) in bytes"""
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
        raise ValueError(f"{name}: a uint8 tensor on the GPU is taken")
    single = t.dim() == 3
    b = t.unsqueeze(0) if single else t
    if b.dim() != 4:
        raise ValueError(f"{name}: [N, H, W, C] or [H, W, C] is taken, got {tuple(t.shape)}")
    n, h, w, c = b.shape
    if b.stride(3) != 1 or (w > 1 and b.stride(2) != c) or n < 1 or h < 1 or w < 1:
        raise ValueError(f"{name}: the pixels of a row must be packed (strides (.., {c}, 1)), got {tuple(b.stride())}")
    if h > 1 and b.stride(1) < w * c or n > 1 and b.stride(0) < 0:
        raise ValueError(f"{name}: rows overlap, strides {tuple(b.stride())}")
    return b, single, n, h, w, c, (b.stride(1) if h > 1 else w * c), (b.stride(0) if n > 1 else 0)


def to_bgr_device(src, encoding: str | None = None, out=None):
    """toCvCopy(BGR8) of [N, H, W, C] / [H, W, C] frames on the GPU (C = 1, 3 or 4: mono8, bgr8 / rgb8, bgra8 / rgba8; strided views
    of packed pixels are taken).  out: a [N, H, W, 3] / [H, W, 3] uint8 tensor on the same GPU to write (strided rows allowed),
    or None for a new one.  Returns out."""
    import torch

    s, single, n, h, w, c, sstride, sfstride = _frames(src, "to_bgr_device")
    encoding = encoding or _ENC_OF_CHANNELS.get(c, "")
    if _lib.ENC_BYTES_PER_PIXEL.get(encoding) != c or encoding not in ("mono8", "bgr8", "rgb8", "bgra8", "rgba8"):
        raise ValueError(f"to_bgr_device: {c} channels do not make {encoding!r}")
    if out is None:
        out = torch.empty((n, h, w, 3) if not single else (h, w, 3), dtype=torch.uint8, device=src.device)
    o, _, on, oh, ow, oc, dstride, dfstride = _frames(out, "to_bgr_device(out)")
    if (on, oh, ow, oc) != (n, h, w, 3):
        raise ValueError(f"to_bgr_device: out is {tuple(out.shape)} for {n} frames of {h} x {w}")
    torch.cuda.current_stream(src.device).synchronize()
    rc = _lib.load().fid_to_bgr_device(s.data_ptr(), n, w, h, sstride, sfstride, _lib.ENC[encoding], o.data_ptr(), dstride, dfstride)
    if rc != _lib.FID_OK:
        raise FidError(rc, "fid_to_bgr_device")
    return out


def draw_detected_markers_device(bgr, corners, ids=None, flags: int = 0):
    """draw_detected_markers in place on [N, H, W, 3] / [H, W, 3] BGR frames on the GPU (strided rows and frames allowed).  corners:
    for one frame an (n, 4, 2) array; for N frames a sequence of N such arrays (ids likewise, one array per frame, or None).
    Returns bgr."""
    import torch

    b, single, n, h, w, c, stride, fstride = _frames(bgr, "draw_detected_markers_device")
    if c != 3:
        raise ValueError("draw_detected_markers_device takes 3-channel BGR frames")
    per = [corners] if single else list(corners)
    pid = [ids] if single else (list(ids) if ids is not None else [None] * len(per))
    if len(per) != n or len(pid) != n:
        raise ValueError(f"draw_detected_markers_device: markers of {len(per)} frames for {n} frames")
    per = [np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 8) for q in per]
    cnt = np.array([len(q) for q in per], dtype=np.int32)
    cap = max(int(cnt.max()), 1)
    mk = np.zeros(n * cap, _MARKER)
    for f, q in enumerate(per):
        mk["corners"][f * cap:f * cap + len(q)] = q
        if pid[f] is not None:
            mk["id"][f * cap:f * cap + len(q)] = np.asarray(pid[f], dtype=np.int32).reshape(-1)[:len(q)]
    torch.cuda.current_stream(bgr.device).synchronize()
    rc = _lib.load().fid_draw_detected_markers_device(b.data_ptr(), n, w, h, stride, fstride, mk.ctypes.data_as(C.POINTER(FidMarker)), cap,
                                                     cnt.ctypes.data_as(C.POINTER(C.c_int32)), flags)
    if rc != _lib.FID_OK:
        raise FidError(rc, "fid_draw_detected_markers_device")
    return bgr
