#!/usr/bin/env python3
"""fid_build_map_cam timed on the device -> profiles/map_build_bench.json.

Host clock around the call (the gather on the host, the uploads, every launch, the status reads and the result copy included), median
of 30, at 64, 256, 1 024 and 4 096 views x 20 markers of a 32- and of a 128-marker map (a wall of 0.125 m markers, one marker fixed,
plumb-bob, the header's default options).  The views are copies of 64 generated ones (tests/map_build_cases.py's generator), each cut to
the 20 markers nearest the image centre.  Recorded beside the times: trials and microseconds per trial, the share of k_build_reduce
and of the factor (k_build_panel + k_build_update) in the kernel time, from one rocprofv3 --kernel-trace --stats run of its own
(a child process that makes one call per size), and the NumPy restatement's time for the smallest size on the same host.
No target is set: nobody has measured this before.

    python tools/gpu_map_build_bench.py [--out profiles/map_build_bench.json] [--reps 30]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import map_build_cases as mc  # noqa: E402
import map_build_restatement as mb  # noqa: E402
from fiducials_amd import _lib, camera  # noqa: E402
from fiducials_amd.detector import MAP_ENTRY_DTYPE, ArucoDetector  # noqa: E402

MARKER_DT = np.dtype([("id", "<i4"), ("corners", "<f4", (8,))])
SIZES = (64, 256, 1024, 4096)
MAPS = {32: (8, (8, 8), (0.8, 0.95)), 128: (16, (16, 4), (0.8, 0.95))}  # markers: (columns, the 64 views' grid, distance)
PER_VIEW = 20


def views_of(n_markers: int):
    """64 views x 20 markers of the map, the generating case beside them."""
    cols, grid, dist = MAPS[n_markers]
    e = mc.grid_board(n_markers, cols)
    views, poses = mc.wall_views(e, 64, "plumb_bob", 900 + n_markers, dist=dist, spread=1.0, grid=grid, tilt_deg=(15.0, 35.0), min_area=600.0)
    cut = []
    for corners, ids in views:
        order = np.argsort(np.abs(corners.reshape(-1, 4, 2).mean(axis=1) - (mc.CX, mc.CY)).sum(axis=1))[:PER_VIEW]
        order.sort()
        cut.append((corners[order].copy(), ids[order].copy()))
    return mc._case(e, cut, poses, "plumb_bob", [int(e["id"][n_markers // 2])])


def pack(views):
    mk = np.zeros((len(views), PER_VIEW), MARKER_DT)
    n = np.zeros(len(views), np.int32)
    for v, (corners, ids) in enumerate(views):
        n[v] = len(ids)
        mk["id"][v, :len(ids)] = ids
        mk["corners"][v, :len(ids)] = corners.reshape(-1, 8)
    return mk, n


def call(det, c, mk, n):
    L = det._L
    opts = _lib.FidBuildOpts()
    L.fid_default_build_opts(C.byref(opts))
    opts.fiducial_len = c["fiducial_len"]
    k = c["k16"]
    cam = camera.Camera(c["model"], [[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]], k[4:9])
    fx = np.ascontiguousarray(c["fixed"], dtype=MAP_ENTRY_DTYPE)
    out = np.zeros(1, _lib.BUILD_OUT_DTYPE)
    mout = np.zeros(256, _lib.BUILD_MARKER_DTYPE)
    n_m = C.c_int32(0)
    t0 = time.perf_counter()
    rc = L.fid_build_map_cam(det._ctx, C.byref(cam.c), mk.ctypes.data, n.ctypes.data, len(n), PER_VIEW, fx.ctypes.data, len(fx), C.byref(opts), out.ctypes.data,
                             mout.ctypes.data, len(mout), C.byref(n_m), None)
    t1 = time.perf_counter()
    assert rc == _lib.FID_OK, L.fid_last_error(det._ctx)
    return (t1 - t0) * 1e3, out[0]


def one_call_per_size():
    """The child of the rocprofv3 run: one call per map and size."""
    det = ArucoDetector(dictionary=6, max_width=640, max_height=480)
    for n_markers in MAPS:
        c = views_of(n_markers)
        for size in SIZES:
            call(det, c, *pack(c["views"] * (size // 64)))


def kernel_shares():
    """Shares of the k_build_* kernels in the kernel time of one call per size, from rocprofv3's kernel statistics; None with the
    reason where the profiler or its file is not there."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--child"],
                           capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"error": "rocprofv3 rc %d, %d stats files: %s" % (r.returncode, len(files), (r.stderr or "")[-200:])}
        tot = {}
        with open(files[0]) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
                for key in ("k_build_reduce", "k_build_panel", "k_build_update", "k_build_blocks", "k_build_schur", "k_build_solve", "k_build_eval", "k_build_accept",
                            "k_build_prep", "k_build_cov", "k_build_finish", "k_map_pose", "k_pose"):
                    if key + "<" in name or name.startswith(key) or (" " + key) in name:
                        tot[key] = tot.get(key, 0.0) + ns
                        break
        s = sum(tot.values())
        return {"kernel_ns": {k: int(v) for k, v in sorted(tot.items())},
                "share_reduce": round(tot.get("k_build_reduce", 0.0) / s, 4) if s else None,
                "share_factor": round((tot.get("k_build_panel", 0.0) + tot.get("k_build_update", 0.0)) / s, 4) if s else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_build_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    if args.child:
        return one_call_per_size()
    det = ArucoDetector(dictionary=6, max_width=640, max_height=480)
    rows, numpy_row = [], None
    for n_markers in MAPS:
        c = views_of(n_markers)
        for size in SIZES:
            mk, n = pack(c["views"] * (size // 64))
            ms = []
            for rep in range(args.reps + 3):
                t, out = call(det, c, mk, n)
                if rep >= 3:
                    ms.append(t)
            med = statistics.median(ms)
            rows.append({"map_markers": n_markers, "views": size, "markers_per_view": PER_VIEW, "in_the_solve": int(out["n_markers"]), "median_ms": round(med, 4),
                         "min_ms": round(min(ms), 4), "trials": int(out["n_iter"]), "us_per_trial": round(1e3 * med / max(int(out["n_iter"]), 1), 2),
                         "status": int(out["status"]), "rms_px": float(out["rms"])})
            print(rows[-1], flush=True)
        if numpy_row is None:
            t0 = time.perf_counter()
            ref = mb.build(c["model"], c["k16"], c["views"], c["fixed"], c["fiducial_len"])
            numpy_row = {"map_markers": n_markers, "views": 64, "seconds": round(time.perf_counter() - t0, 3), "iterations": int(ref["iterations"]),
                         "rms_px": float(ref["rms"])}
    doc = {"what": "fid_build_map_cam, host clock around the call, median of %d; plumb-bob, one marker fixed, default options" % args.reps,
           "device_text_sha256": _lib.device_text_sha256(), "rows": rows, "numpy_restatement": numpy_row,
           "kernel_shares": None if args.no_profile else kernel_shares()}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"numpy_restatement": numpy_row, "kernel_shares": doc["kernel_shares"]}))


if __name__ == "__main__":
    main()
