#!/usr/bin/env python3
"""What the pose covariance costs (run on the GPU box): fid_pose_cam against fid_pose_cov_cam on the same markers, 256 x 20 markers
(a full batch's poses in one call) and 1 x 20 markers (the single-frame shape), by the host clock around the call -- both return when
the records are in host memory.  After warm-up the two variants alternate call by call, so clock drift and whatever else the
machine does fall on both alike; the figure is the median of the calls, with p10 / p90 beside it.  The difference covers k_pose_cov
behind k_pose (one more Jacobian at the returned pose and the 6 x 6 algebra, a launch of its own) and the copy of 592 bytes per marker.
A third figure is the remembered road (in_stream): fid_detect + fid_pose_last_cam against fid_detect + fid_pose_last_cov_cam on one
1920 x 1080 frame of 20 markers, two contexts that each remember their own form.
Usage: python tools/gpu_pose_cov_bench.py [--out profiles/pose_cov_bench.json] [--calls 60]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from fiducials_amd import _lib, synth  # noqa: E402
from fiducials_amd.camera import Camera  # noqa: E402
from fiducials_amd.detector import POSE_COV_DTYPE, ArucoDetector  # noqa: E402
from fiducials_amd.dictionary import get_predefined_dictionary  # noqa: E402

W, H, LEN = 1920, 1080, 0.14


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64)) * 1e6
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(ts[len(ts) // 10]), 2), "p90_us": round(float(ts[(9 * len(ts)) // 10]), 2),
            "calls": len(ts)}


def one_shape(det, frames, calls):
    d = get_predefined_dictionary("DICT_5X5_250")
    corners = np.concatenate([synth.make_frame(d, 3 + f % 4, W, H, n_markers=20).corners for f in range(frames)]).astype(np.float32).reshape(-1, 8)
    n = len(corners)
    K = synth.K_DEFAULT.copy()
    camera = Camera(_lib.CAM_PLUMB_BOB, K, np.array([0.05, -0.02, 0.001, -0.0005, 0.0]))
    mk = (_lib.FidMarker * n)()
    for i in range(n):
        mk[i].id = i % 50
        for j in range(8):
            mk[i].corners[j] = float(corners[i, j])
    out = (_lib.FidPoseOut * n)()
    cov = np.zeros(n, POSE_COV_DTYPE)
    L, ctx, cam = det._L, det._ctx, C.byref(camera.c)
    plain = lambda: L.fid_pose_cam(ctx, cam, mk, None, n, LEN, out)  # noqa: E731
    with_cov = lambda: L.fid_pose_cov_cam(ctx, cam, mk, None, n, LEN, out, 1.0, cov.ctypes.data)  # noqa: E731
    for _ in range(10):
        assert plain() == _lib.FID_OK and with_cov() == _lib.FID_OK
    assert (cov["status"] == 0).all()
    tp, tc = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        plain()
        t1 = time.perf_counter()
        with_cov()
        t2 = time.perf_counter()
        tp.append(t1 - t0)
        tc.append(t2 - t1)
    a, b = spread(tp), spread(tc)
    return {"markers": n, "fid_pose_cam": a, "fid_pose_cov_cam": b, "added_us_median": round(b["median_us"] - a["median_us"], 2),
            "added_us_per_marker": round((b["median_us"] - a["median_us"]) / n, 4)}


def in_stream(calls):
    """The remembered road on one 1920 x 1080 frame of 20 markers: fid_detect + fid_pose_last_cam on a context that remembers the
    camera, against fid_detect + fid_pose_last_cov_cam on one that remembers the camera and sigma_px (k_pose_cov rides in the detect
    call's stream, the _cov call copies the records out), alternating."""
    d = get_predefined_dictionary("DICT_5X5_250")
    img = np.ascontiguousarray(synth.make_frame(d, 3, W, H, n_markers=20).image)
    camera = Camera(_lib.CAM_PLUMB_BOB, synth.K_DEFAULT.copy(), np.array([0.05, -0.02, 0.001, -0.0005, 0.0]))
    dets = [ArucoDetector("DICT_5X5_250", max_width=W, max_height=H, max_batch=1, max_markers=64) for _ in range(2)]
    cov = np.zeros(64, POSE_COV_DTYPE)
    L, cam = dets[0]._L, C.byref(camera.c)

    def call(det, with_cov):
        rc = L.fid_detect(det._ctx, img.ctypes.data, W, H, W, _lib.ENC["mono8"], det._out, 64, det._n)
        rc |= L.fid_pose_last_cov_cam(det._ctx, cam, LEN, det._poses, 64, 1.0, cov.ctypes.data) if with_cov else L.fid_pose_last_cam(det._ctx, cam, LEN, det._poses, 64)
        return rc

    for _ in range(10):
        assert call(dets[0], False) == _lib.FID_OK and call(dets[1], True) == _lib.FID_OK
    assert dets[1]._n[0] == 20 and (cov["status"][:20] == 0).all()
    tp, tc = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        call(dets[0], False)
        t1 = time.perf_counter()
        call(dets[1], True)
        t2 = time.perf_counter()
        tp.append(t1 - t0)
        tc.append(t2 - t1)
    for det in dets:
        det.close()
    a, b = spread(tp), spread(tc)
    return {"markers": 20, "fid_detect+fid_pose_last_cam": a, "fid_detect+fid_pose_last_cov_cam": b, "added_us_median": round(b["median_us"] - a["median_us"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cov_bench.json"))
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    assert a.calls >= 30
    det = ArucoDetector("DICT_5X5_250", max_width=640, max_height=480, max_batch=1, max_markers=32)
    doc = {"device_text_sha256": _lib.device_text_sha256(), "what": "host clock around the call, the two variants alternating; median of the calls",
           "shapes": {"256x20": one_shape(det, 256, a.calls), "1x20": one_shape(det, 1, a.calls)}, "in_stream_1x20": in_stream(a.calls)}
    det.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
