#!/usr/bin/env python3
"""Marker-image timings (run on the GPU box), one JSON line:
  * the compressed-frame callback of FiducialsNode on one 1920x1080 JPEG with 20 markers, as the node makes its calls: with
    ~publish_images off (fid_jpeg_decode MONO8 -> fid_detect_device) and on (decode BGR8 -> fid_detect_device(BGR8) ->
    fid_jpeg_marker_image into host memory);
  * fid_draw_detected_markers_device on a batch of B 1920x1080 BGR frames in HBM, 20 markers each (markers uploaded per call).
Usage: python tools/gpu_overlay_bench.py [batch] [iterations]"""
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import torch  # noqa: E402

torch.cuda.init()
from fiducials_amd import _lib, overlay, synth  # noqa: E402
from fiducials_amd import jpeg as fj  # noqa: E402
from fiducials_amd.detector import ArucoDetector  # noqa: E402
from fiducials_amd.dictionary import get_predefined_dictionary  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
IT = int(sys.argv[2]) if len(sys.argv) > 2 else 50
W, H = 1920, 1080
L = _lib.load()


def stats(ts):
    ts = np.sort(np.array(ts) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 4), "p10_ms": round(float(ts[len(ts) // 10]), 4), "p90_ms": round(float(ts[(9 * len(ts)) // 10]), 4)}


d = get_predefined_dictionary("DICT_5X5_250")
fr = synth.make_frame(d, 3, W, H, n_markers=20)
b = io.BytesIO()
Image.fromarray(np.stack([fr.image] * 3, -1)).save(b, "JPEG", quality=80, subsampling=2)
data = b.getvalue()
det = ArucoDetector(d, device=0, max_width=W, max_height=H)
dec = fj.JpegDecoder(max_width=W, max_height=H)
files = (C.c_void_p * 1)(C.cast(C.c_char_p(data), C.c_void_p))
sizes = (C.c_int64 * 1)(len(data))
mk = (_lib.FidMarker * 1024)()
n = C.c_int32(0)
img = np.empty((H, W, 3), np.uint8)
w_, h_, s_, fs_ = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()


def callback(publish_images):
    enc = _lib.ENC["bgr8" if publish_images else "mono8"]
    assert L.fid_jpeg_decode(dec._ctx, files, sizes, 1, enc, None, 0) == 0
    p = L.fid_jpeg_device_ptr(dec._ctx, C.byref(w_), C.byref(h_), C.byref(s_), C.byref(fs_))
    assert L.fid_detect_device(det._ctx, C.c_void_p(p), 1, w_, h_, s_, fs_, enc, mk, 1024, C.byref(n)) == 0
    if publish_images:
        assert L.fid_jpeg_marker_image(dec._ctx, 0, enc, mk, n.value, 0, img.ctypes.data_as(C.c_void_p), C.c_int64(img.nbytes)) == 0
    return n.value


out = {"frame": [W, H], "jpeg_bytes": len(data)}
for on in (False, True):
    for _ in range(5):
        found = callback(on)
    ts = []
    for _ in range(IT):
        t = time.perf_counter()
        callback(on)
        ts.append(time.perf_counter() - t)
    out["compressed_callback_image_" + ("on" if on else "off")] = dict(stats(ts), markers=found)
det.close()
dec.close()

# fid_draw_detected_markers_device on B frames
frames = torch.zeros((B, H, W, 3), dtype=torch.uint8, device="cuda")
quads = [q.astype(np.float32) for q in [fr.corners] * B]
torch.cuda.synchronize()
for _ in range(3):
    overlay.draw_detected_markers_device(frames, quads)
ts = []
for _ in range(max(IT // 5, 5)):
    t = time.perf_counter()
    overlay.draw_detected_markers_device(frames, quads)
    ts.append(time.perf_counter() - t)
out["draw_device_batch"] = dict(stats(ts), frames=B, markers_per_frame=len(fr.corners))
M = len(fr.corners)
mkb = (_lib.FidMarker * (B * M))()
for f in range(B):
    for i in range(M):
        for j in range(8):
            mkb[f * M + i].corners[j] = float(fr.corners[i].reshape(8)[j])
cnt = (C.c_int32 * B)(*([M] * B))
ts = []
for _ in range(max(IT // 5, 5)):
    t = time.perf_counter()
    assert L.fid_draw_detected_markers_device(C.c_void_p(frames.data_ptr()), B, W, H, W * 3, W * H * 3, mkb, M, cnt, 0) == 0
    ts.append(time.perf_counter() - t)
out["draw_device_batch_abi_only"] = dict(stats(ts), frames=B)
ts = []
for _ in range(max(IT // 5, 5)):
    t = time.perf_counter()
    assert L.fid_draw_detected_markers_device(C.c_void_p(frames.data_ptr()), B, W, H, W * 3, W * H * 3, mkb, M, cnt, 1) == 0
    ts.append(time.perf_counter() - t)
out["draw_device_batch_first_corner_square"] = dict(stats(ts), frames=B)
src = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ts = []
for _ in range(max(IT // 5, 5)):
    t = time.perf_counter()
    overlay.to_bgr_device(src.unsqueeze(-1), "mono8", out=frames)
    ts.append(time.perf_counter() - t)
out["to_bgr_device_batch_mono8"] = dict(stats(ts), frames=B, GB_per_s=round(B * W * H * 4 / 1e9 / (np.median(ts)), 1))
print(json.dumps(out))
