#!/usr/bin/env python3
"""What the consensus map pose costs (run on the GPU box): k_map_pose_robust against k_map_pose on the same markers, where they lie
after a detect call -- fid_map_pose_robust_last_cam against fid_map_pose_last_cam with FID_NO_POSE_AHEAD set, so that every call
launches its kernel for the whole batch, copies the records out and returns when they are in host memory.  Shapes: 256 frames x 20
mapped markers in one launch with a truthful map (0 outliers) and with a map in which two entries have exchanged places (2
outliers; the plain kernel poses from all 20 either way), and one frame x 20.  After warm-up the two calls alternate, so clock
drift and whatever else the machine does fall on both alike; the figure is the median of the calls by the host clock, with p10 /
p90 beside it.  Both calls carry the same launch, copy and synchronisation overhead, which is most of the one-frame figure.
Usage: python tools/gpu_map_robust_bench.py [--out profiles/map_robust_bench.json] [--calls 60]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ["FID_NO_POSE_AHEAD"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from fiducials_amd import _lib, synth  # noqa: E402
from fiducials_amd.camera import Camera  # noqa: E402
from fiducials_amd.detector import MAP_POSE_DTYPE, MAP_ROBUST_DTYPE, ArucoDetector, map_entries  # noqa: E402
from fiducials_amd.dictionary import get_predefined_dictionary  # noqa: E402

W, H, LEN, PITCH, N = 640, 480, 0.08, 0.11, 20
K = np.array([[466.7, 0, 320.0], [0, 466.7, 240.0], [0, 0, 1.0]])
FACING = np.diag([1.0, -1.0, -1.0])


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64)) * 1e6
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(ts[len(ts) // 10]), 2), "p90_us": round(float(ts[(9 * len(ts)) // 10]), 2),
            "calls": len(ts)}


def board():
    k = np.arange(N)
    xy = np.stack([(k % 5) * PITCH - 2 * PITCH, (k // 5) * PITCH - 1.5 * PITCH, np.zeros(N)], axis=1)
    return map_entries(40 + k, LEN, np.broadcast_to(np.eye(3), (N, 3, 3)), xy)


def frames_of(e, count):
    d = get_predefined_dictionary("DICT_5X5_250")
    views = []
    for s in range(4):
        R = synth._rodrigues(np.array([0.15 * (s - 1.5), 0.1 * (s % 2), 0.05 * s])) @ FACING
        fr = synth.make_aruco_board_frame(d, e["id"], [(float(x["len"]), x["R"], x["t"]) for x in e], K, R, np.array([0.01, -0.01, 0.95 + 0.05 * s]), 7 + s, W, H)
        views.append(fr.image)
    return np.ascontiguousarray(np.stack([views[f % 4] for f in range(count)]))


def one_shape(frames, e, lying, calls, inlier_px):
    F = len(frames)
    det = ArucoDetector("DICT_5X5_250", max_width=W, max_height=H, max_batch=F, max_markers=32)
    camera = Camera(_lib.CAM_PLUMB_BOB, K, ())
    opts = _lib.FidMapRobustOpts(inlier_px, 2, 0)
    out, rob = np.zeros(F, MAP_POSE_DTYPE), np.zeros(F, MAP_ROBUST_DTYPE)
    L, ctx, cam = det._L, det._ctx, C.byref(camera.c)
    plain = lambda: L.fid_map_pose_last_cam(ctx, cam, out.ctypes.data, F)  # noqa: E731
    robust = lambda: L.fid_map_pose_robust_last_cam(ctx, cam, C.byref(opts), out.ctypes.data, rob.ctypes.data, F)  # noqa: E731
    doc = {}
    for name, m, n_out in (("0_outliers", e, 0), ("2_outliers", lying, 2)):
        det.set_map(m)
        res = det.detect_markers_batch(frames)
        assert all(len(r[1]) == N for r in res), [len(r[1]) for r in res][:8]
        for _ in range(10):
            assert plain() == _lib.FID_OK and robust() == _lib.FID_OK
        assert (rob["status"] == 0).all() and (rob["n_outliers"] == n_out).all() and (rob["n_used"] == N).all(), (rob["status"], rob["n_outliers"])
        tp, tr = [], []
        for _ in range(calls):
            t0 = time.perf_counter()
            plain()
            t1 = time.perf_counter()
            robust()
            t2 = time.perf_counter()
            tp.append(t1 - t0)
            tr.append(t2 - t1)
        a, b = spread(tp), spread(tr)
        doc[name] = {"frames": F, "markers_per_frame": N, "rounds": sorted(set(int(v) for v in rob["rounds"])), "fid_map_pose_last_cam": a,
                     "fid_map_pose_robust_last_cam": b, "added_us_median": round(b["median_us"] - a["median_us"], 2),
                     "ratio_median": round(b["median_us"] / a["median_us"], 3)}
    det.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_robust_bench.json"))
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--inlier-px", type=float, default=_lib.MAP_ROBUST_INLIER_PX)
    a = ap.parse_args()
    assert a.calls >= 30
    e = board()
    lying = e.copy()
    lying["R"][[3, 16]], lying["t"][[3, 16]] = e["R"][[16, 3]], e["t"][[16, 3]]
    doc = {"device_text_sha256": _lib.device_text_sha256(),
           "what": "host clock around the call (launch for the whole batch + copy + synchronise), FID_NO_POSE_AHEAD set, the two calls alternating; "
                   "median of the calls",
           "inlier_px": a.inlier_px, "shapes": {"256x20": one_shape(frames_of(e, 256), e, lying, a.calls, a.inlier_px),
                                                  "1x20": one_shape(frames_of(e, 1), e, lying, a.calls, a.inlier_px)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
