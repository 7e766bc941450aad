#!/usr/bin/env python3
"""What the diamond calls cost (run on the GPU box): fid_diamonds_last on the frames of a detect call, with and without the refinement,
and fid_charuco_last_cam by homographies (a 5 x 4 board, the figure DESIGN §28 gives) beside it in the same run.  Shapes: one frame and
256 frames of three diamonds and eight loose markers at 640 x 480; one frame of 64 diamonds -- 256 markers, both limits -- at
1920 x 1440.  Every call launches for the whole batch, copies its records out and returns when they are in host memory; the figure is
the median of the calls by the host clock, with p10 / p90 beside it.  After warm-up the calls alternate, so clock drift falls on all
alike.
Usage: python tools/gpu_diamond_bench.py [--out profiles/diamond_bench.json] [--calls 60]"""
import argparse
import ctypes as C
import functools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from fiducials_amd import _lib, synth  # noqa: E402
from fiducials_amd.charuco import CharucoBoard, CharucoDiamond  # noqa: E402
from fiducials_amd.detector import CHARUCO_CORNER_DTYPE, DIAMOND_DTYPE, ArucoDetector, default_params  # noqa: E402
from fiducials_amd.dictionary import get_predefined_dictionary  # noqa: E402

W, H = 640, 480
K = np.array([[466.7, 0, 320.0], [0, 466.7, 240.0], [0, 0, 1.0]])
FACING = np.diag([1.0, -1.0, -1.0])
SQUARE, MARKER = 0.04, 0.024
RATE = SQUARE / MARKER


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64)) * 1e6
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(ts[len(ts) // 10]), 2), "p90_us": round(float(ts[(9 * len(ts)) // 10]), 2),
            "calls": len(ts)}


def _pose(centre, tilt, dist, shift_px, Kc):
    R = synth._rodrigues(np.asarray(tilt, float)) @ FACING
    return R, np.array([shift_px[0] * dist / Kc[0, 0], shift_px[1] * dist / Kc[1, 1], dist]) - R @ np.asarray(centre, float)


@functools.lru_cache(maxsize=None)
def small_frame(seed):
    """three diamonds in a row (markers of 30 px) above eight loose markers in two rows"""
    d = get_predefined_dictionary(7)
    dia = [(CharucoDiamond((4 * i, 4 * i + 1, 4 * i + 2, 4 * i + 3), SQUARE, MARKER), 0.02 * (i - 1 + seed % 3), (-205.0 + 205.0 * i, -130.0)) for i in range(3)]
    diamonds = [(b, *_pose(b.centre, (tilt, -tilt, 0.0), 0.37, shift, K)) for b, tilt, shift in dia]
    loose = [(20 + i, MARKER, *_pose((0.75 * MARKER, 0.75 * MARKER, 0.0), (0.0, 0.03 * (i % 3), 0.0), 0.37, (-240.0 + 160.0 * (i % 4), 40.0 + 120.0 * (i // 4)), K))
             for i in range(8)]
    return synth.make_diamond_frame(d, diamonds, K, seed, loose=loose, width=W, height=H).image


def large_frame():
    """64 diamonds of 256 markers at 1920 x 1440: one rendered 240 x 180 tile (markers of 32 px), eight by eight.  Ids play no part in the
    matching, so the tiles may all carry the same four."""
    d = get_predefined_dictionary(7)
    Kt = np.array([[466.7, 0, 120.0], [0, 466.7, 90.0], [0, 0, 1.0]])
    b = CharucoDiamond((0, 1, 2, 3), SQUARE, MARKER)
    tile = synth.make_diamond_frame(d, [(b, *_pose(b.centre, (0.0, 0.0, 0.0), 0.35, (0.0, 0.0), Kt))], Kt, 3, width=240, height=180).image
    return np.ascontiguousarray(np.tile(tile, (8, 8)))


def time_calls(fns, calls):
    for _ in range(10):
        for fn in fns.values():
            assert fn() == _lib.FID_OK
    ts = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: spread(v) for k, v in ts.items()}


def diamond_fns(det, F):
    L, ctx = det._L, det._ctx
    cap = _lib.DIAMOND_MAX_PER_FRAME
    out, n = np.zeros(F * cap, DIAMOND_DTYPE), np.zeros(F, np.int32)
    o1, o0 = det._diamond_opts(RATE, None, True), det._diamond_opts(RATE, None, False)
    return n, {"fid_diamonds_last": lambda: L.fid_diamonds_last(ctx, C.byref(o1), out.ctypes.data, cap, n.ctypes.data),
               "fid_diamonds_last, refine = 0": lambda: L.fid_diamonds_last(ctx, C.byref(o0), out.ctypes.data, cap, n.ctypes.data)}


def small_shape(F, calls):
    views = [small_frame(11 + s) for s in range(4)]
    frames = np.ascontiguousarray(np.stack([views[f % 4] for f in range(F)]))
    det = ArucoDetector(7, max_width=W, max_height=H, max_batch=F, max_markers=32)
    found = [len(r[1]) for r in det.detect_markers_batch(frames)]
    n, fns = diamond_fns(det, F)
    res = time_calls(fns, calls)
    det.close()
    assert (n == 3).all(), n
    return {"frames": F, "markers_found": [min(found), max(found)], "diamonds": [int(n.min()), int(n.max())], **res}


def large_shape(calls):
    frame = large_frame()
    # markers of 32 px in a frame of 1920: below the default minMarkerPerimeterRate (0.1 of the larger side); one threshold window
    # keeps the candidates of 256 markers inside the default limits
    p = default_params()
    p.minMarkerPerimeterRate = 0.06
    p.adaptiveThreshWinSizeMin = p.adaptiveThreshWinSizeMax = 13
    det = ArucoDetector(7, params=p, max_width=frame.shape[1], max_height=frame.shape[0], max_batch=1, max_markers=256)
    found = len(det.detect_markers(frame)[1])
    n, fns = diamond_fns(det, 1)
    res = time_calls(fns, calls)
    det.close()
    return {"frames": 1, "width": int(frame.shape[1]), "height": int(frame.shape[0]), "markers_found": found, "diamonds": int(n[0]), **res}


@functools.lru_cache(maxsize=None)
def charuco_views():
    board = CharucoBoard(5, 4, SQUARE, MARKER)
    d = get_predefined_dictionary(7)
    centre = np.array([board.squares_x * board.square_len / 2, board.squares_y * board.square_len / 2, 0.0])
    views = []
    for s in range(4):
        R = synth._rodrigues(np.array([0.12 * (s - 1.5), 0.1 * (s % 2), 0.05 * s])) @ FACING
        views.append(synth.make_charuco_frame(d, board, K, R, np.array([0.0, 0.0, 0.36 + 0.02 * s]) - R @ centre, 7 + s, W, H).image)
    return board, views


def charuco_shape(F, calls):
    """fid_charuco_last_cam by homographies on tools/gpu_charuco_bench.py's frames"""
    board, views = charuco_views()
    frames = np.ascontiguousarray(np.stack([views[f % 4] for f in range(F)]))
    det = ArucoDetector(7, max_width=W, max_height=H, max_batch=F, max_markers=32)
    det.set_charuco_board(board)
    det.detect_markers_batch(frames)
    nc = board.n_corners
    corners, n = np.zeros(F * nc, CHARUCO_CORNER_DTYPE), np.zeros(F, np.int32)
    L, ctx = det._L, det._ctx
    res = time_calls({"fid_charuco_last_cam, homographies": lambda: L.fid_charuco_last_cam(ctx, None, 2, corners.ctypes.data, nc, n.ctypes.data)}, calls)
    det.close()
    return {"frames": F, "corners_kept": [int(n.min()), int(n.max())], **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diamond_bench.json"))
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    assert a.calls >= 30
    doc = {"device_text_sha256": _lib.device_text_sha256(),
           "what": "host clock around the call (launches for the whole batch + copy + synchronise), the calls alternating; median of the calls",
           "3 diamonds + 8 loose markers, 640 x 480": {"1": small_shape(1, a.calls), "256": small_shape(256, a.calls)},
           "64 diamonds of 256 markers, 1920 x 1440": large_shape(a.calls),
           "5 x 4 ChArUco board, 640 x 480": {"1": charuco_shape(1, a.calls), "256": charuco_shape(256, a.calls)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
