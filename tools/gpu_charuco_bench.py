#!/usr/bin/env python3
"""What the ChArUco calls cost (run on the GPU box): fid_charuco_last_cam by either route and fid_charuco_pose_last_cam on the frames of
a detect call, with fid_map_pose_last_cam (the board's markers as the map, FID_NO_POSE_AHEAD set so that every call launches its kernel)
beside them in the same run.  Shapes: one frame and 256 frames of a 5 x 4 board at 640 x 480.  Every call launches for the whole batch,
copies its records out and returns when they are in host memory; the figure is the median of the calls by the host clock, with p10 /
p90 beside it.  After warm-up the calls alternate, so clock drift falls on all alike.
Usage: python tools/gpu_charuco_bench.py [--out profiles/charuco_bench.json] [--calls 60]"""
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
from fiducials_amd.charuco import CharucoBoard  # noqa: E402
from fiducials_amd.detector import CHARUCO_CORNER_DTYPE, CHARUCO_POSE_DTYPE, MAP_POSE_DTYPE, ArucoDetector  # noqa: E402
from fiducials_amd.dictionary import get_predefined_dictionary  # noqa: E402

W, H = 640, 480
K = np.array([[466.7, 0, 320.0], [0, 466.7, 240.0], [0, 0, 1.0]])
FACING = np.diag([1.0, -1.0, -1.0])


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64)) * 1e6
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(ts[len(ts) // 10]), 2), "p90_us": round(float(ts[(9 * len(ts)) // 10]), 2),
            "calls": len(ts)}


def frames_of(board, count):
    d = get_predefined_dictionary(7)
    centre = np.array([board.squares_x * board.square_len / 2, board.squares_y * board.square_len / 2, 0.0])
    views = []
    for s in range(4):
        R = synth._rodrigues(np.array([0.12 * (s - 1.5), 0.1 * (s % 2), 0.05 * s])) @ FACING
        views.append(synth.make_charuco_frame(d, board, K, R, np.array([0.0, 0.0, 0.36 + 0.02 * s]) - R @ centre, 7 + s, W, H).image)
    return np.ascontiguousarray(np.stack([views[f % 4] for f in range(count)]))


def one_shape(board, F, calls):
    frames = frames_of(board, F)
    det = ArucoDetector(7, max_width=W, max_height=H, max_batch=F, max_markers=32)
    camera = Camera(_lib.CAM_PLUMB_BOB, K, ())
    det.set_charuco_board(board)
    det.set_map(board.as_map_entries())
    res = det.detect_markers_batch(frames)
    found = [len(r[1]) for r in res]
    nc = board.n_corners
    corners, n = np.zeros(F * nc, CHARUCO_CORNER_DTYPE), np.zeros(F, np.int32)
    cposes, mposes = np.zeros(F, CHARUCO_POSE_DTYPE), np.zeros(F, MAP_POSE_DTYPE)
    L, ctx, cam = det._L, det._ctx, C.byref(camera.c)
    fns = {"fid_charuco_last_cam, homographies": lambda: L.fid_charuco_last_cam(ctx, None, 2, corners.ctypes.data, nc, n.ctypes.data),
           "fid_charuco_last_cam, camera": lambda: L.fid_charuco_last_cam(ctx, cam, 2, corners.ctypes.data, nc, n.ctypes.data),
           "fid_charuco_pose_last_cam": lambda: L.fid_charuco_pose_last_cam(ctx, cam, 2, cposes.ctypes.data, F),
           "fid_map_pose_last_cam": lambda: L.fid_map_pose_last_cam(ctx, cam, mposes.ctypes.data, F)}
    for _ in range(10):
        for fn in fns.values():
            assert fn() == _lib.FID_OK
    assert (cposes["status"] == 0).all() and (mposes["n_markers"] > 0).all(), (cposes["status"], mposes["n_markers"])
    ts = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    det.close()
    return {"frames": F, "markers_found": [min(found), max(found)], "corners_kept": [int(n.min()), int(n.max())], **{k: spread(v) for k, v in ts.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "charuco_bench.json"))
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    assert a.calls >= 30
    board = CharucoBoard(5, 4, 0.04, 0.024)
    doc = {"device_text_sha256": _lib.device_text_sha256(),
           "what": "host clock around the call (launches for the whole batch + copy + synchronise), FID_NO_POSE_AHEAD set, the calls alternating; "
                   "median of the calls; 5 x 4 board, 640 x 480",
           "shapes": {"1": one_shape(board, 1, a.calls), "256": one_shape(board, 256, a.calls)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
