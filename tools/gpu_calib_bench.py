#!/usr/bin/env python3
"""fid_calibrate_map timed on the device -> profiles/calib_bench.json.

Host clock around the call (marker upload, every launch, the status reads and the result copy included), median of 30, at 16, 64, 256
and 1 024 views x 20 markers, plumb-bob with 9 free slots, AUTO start, the header's default options.  The views are copies of one
16-view set (tests/calib_cases.py's generator).  Also the NumPy restatement's time for the 16-view problem on the same host.
No target is set: nobody has measured this before.

    python tools/gpu_calib_bench.py [--out profiles/calib_bench.json] [--reps 30]

--charuco: fid_calibrate_charuco instead -> profiles/calib_charuco_bench.json.  16, 64 and 256 views of a 10 x 9 board (72 chessboard
corners a view), copies of one 16-view set, the same clock and options; beside every size, in the same run, fid_calibrate_map on the
same views' 45 markers (the board as the map, the marker corners projected by the same poses with the same noise).

    python tools/gpu_calib_bench.py --charuco [--out profiles/calib_charuco_bench.json] [--reps 30]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import calib_cases as cc  # noqa: E402
import calib_restatement as cr  # noqa: E402
from fiducials_amd import _lib, camera  # noqa: E402
from fiducials_amd.detector import ArucoDetector  # noqa: E402


def timed(call, reps):
    """median and minimum in ms of reps calls after three that are not counted; call() -> the status"""
    ms = []
    for rep in range(reps + 3):
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        assert rc == _lib.FID_OK, rc
        if rep >= 3:
            ms.append((t1 - t0) * 1e3)
    return statistics.median(ms), min(ms)


def main_charuco(args):
    import charuco_calib_cases as ccc
    model, D, _ = cc.MODELS["plumb_bob"]
    k16 = cc.k16_of(D)
    board, rb = ccc.device_board("10x9"), ccc.rboard("10x9")
    rng = np.random.default_rng(20261023)
    base_pts, base_mk = [], []
    for _ in range(16):
        R, t, uv = cc.view_pose(rng, model, k16, np.concatenate([rb.corner_obj, rb.marker_obj.reshape(-1, 3)]))
        uv = (uv + cc.SIGMA * rng.standard_normal(uv.shape)).astype(np.float32)
        base_pts.append(uv[:rb.n_corners])
        base_mk.append(uv[rb.n_corners:].reshape(-1, 8))
    det = ArucoDetector(dictionary=ccc.DICT, max_width=640, max_height=480)
    det.set_charuco_board(board)
    det.set_map(board.as_map_entries())
    L = det._L
    opts = _lib.FidCalibOpts()
    L.fid_default_calib_opts(C.byref(opts))
    out = np.zeros(1, _lib.CALIB_OUT_DTYPE)
    rows = []
    for copies in (1, 4, 16):
        nv = 16 * copies
        rec = np.zeros((nv, rb.n_corners), _lib.CHARUCO_CORNER_DTYPE)
        mk = np.zeros((nv, rb.n_markers), np.dtype([("id", "<i4"), ("corners", "<f4", (8,))]))
        for v in range(nv):
            rec["id"][v] = np.arange(rb.n_corners)
            rec["x"][v], rec["y"][v] = base_pts[v % 16][:, 0], base_pts[v % 16][:, 1]
            mk["id"][v] = board.ids
            mk["corners"][v] = base_mk[v % 16]
        n_pts, n_mk = np.full(nv, rb.n_corners, np.int32), np.full(nv, rb.n_markers, np.int32)
        row = {"views": nv, "corners_per_view": rb.n_corners, "markers_per_view": rb.n_markers}
        for name, fn, data, n, cap in (("charuco", L.fid_calibrate_charuco, rec, n_pts, rb.n_corners), ("map", L.fid_calibrate_map, mk, n_mk, rb.n_markers)):
            def call():
                cam = camera.Camera(_lib.CAM_PLUMB_BOB, np.eye(3), np.zeros(5))
                return fn(det._ctx, data.ctypes.data, n.ctypes.data, nv, cap, cc.W, cc.H, C.byref(opts), C.byref(cam.c), out.ctypes.data, None)
            med, low = timed(call, args.reps)
            row[name] = {"median_ms": round(med, 4), "min_ms": round(low, 4), "trials": int(out[0]["n_iter"]),
                         "ms_per_trial": round(med / max(int(out[0]["n_iter"]), 1), 5), "status": int(out[0]["status"]), "n_points": int(out[0]["n_points"]),
                         "rms_px": float(out[0]["rms"])}
        rows.append(row)
        print(row, flush=True)
    doc = {"what": "fid_calibrate_charuco (72 corners a view of a 10 x 9 board) and fid_calibrate_map (the same views' 45 markers), host clock around "
                   "the call, median of %d; plumb-bob, 9 free, AUTO start, default options" % args.reps,
           "device_text_sha256": _lib.device_text_sha256(), "rows": rows}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--charuco", action="store_true", help="time fid_calibrate_charuco, with fid_calibrate_map beside it")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "calib_charuco_bench.json" if args.charuco else "calib_bench.json")
    if args.charuco:
        return main_charuco(args)
    cc.SHAPES_LARGE["16x20"] = (16, 20, 5, cc.SIGMA)
    c = cc.case("plumb_bob", "16x20")
    det = ArucoDetector(dictionary=6, max_width=640, max_height=480)
    det.set_map(c["entries"])
    L = det._L
    rows = []
    for copies in (1, 4, 16, 64):
        views = c["views"] * copies
        cap = 20
        mk = np.zeros((len(views), cap), np.dtype([("id", "<i4"), ("corners", "<f4", (8,))]))
        n = np.full(len(views), cap, np.int32)
        for v, (corners, ids) in enumerate(views):
            mk["id"][v] = ids
            mk["corners"][v] = corners.reshape(cap, 8)
        opts = _lib.FidCalibOpts()
        L.fid_default_calib_opts(C.byref(opts))
        out = np.zeros(1, _lib.CALIB_OUT_DTYPE)
        ms = []
        for rep in range(args.reps + 3):
            cam = camera.Camera(_lib.CAM_PLUMB_BOB, np.eye(3), np.zeros(5))
            t0 = time.perf_counter()
            rc = L.fid_calibrate_map(det._ctx, mk.ctypes.data, n.ctypes.data, len(views), cap, cc.W, cc.H, C.byref(opts), C.byref(cam.c), out.ctypes.data, None)
            t1 = time.perf_counter()
            assert rc == _lib.FID_OK, L.fid_last_error(det._ctx)
            if rep >= 3:
                ms.append((t1 - t0) * 1e3)
        med = statistics.median(ms)
        rows.append({"views": len(views), "markers_per_view": cap, "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "trials": int(out[0]["n_iter"]),
                     "ms_per_trial": round(med / max(int(out[0]["n_iter"]), 1), 5), "status": int(out[0]["status"]), "rms_px": float(out[0]["rms"])})
        print(rows[-1], flush=True)
    t0 = time.perf_counter()
    ref = cr.calibrate(c["entries"], c["views"], c["image_size"], c["model"], cc.zero_start(c), c["free"], start="auto")
    numpy_s = time.perf_counter() - t0
    doc = {"what": "fid_calibrate_map, host clock around the call, median of %d; plumb-bob, 9 free, AUTO start, default options" % args.reps,
           "device_text_sha256": _lib.device_text_sha256(), "rows": rows,
           "numpy_restatement_16_views": {"seconds": round(numpy_s, 3), "iterations": int(ref["iterations"]), "rms_px": float(ref["rms"])}}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc["numpy_restatement_16_views"]))


if __name__ == "__main__":
    main()
