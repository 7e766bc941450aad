#!/usr/bin/env python3
"""fid_build_map_robust_cam timed against fid_build_map_cam in the same run -> profiles/map_build_robust_bench.json.

Host clock around the call, median of 30, a 32- and a 128-marker map (tools/gpu_map_build_bench.py's walls and views, 20 markers a
view) at 64 / 256 / 1 024 views, with 0 and with 2 wrong ids a view (two of the view's markers relabelled as markers it does not
show).  The plain call is timed on the same views; with wrong ids in them its answer is wrong, its time is what it is.  Beside the
times: rounds, outliers, and the share of the two new kernels (k_build_place_score, k_build_obs_err) in the kernel time of one
robust call per row, from one rocprofv3 --kernel-trace --stats run of its own (a child process).  No target is set.

    python tools/gpu_map_build_robust_bench.py [--out profiles/map_build_robust_bench.json] [--reps 30]"""
import argparse
import csv
import ctypes as C
import glob
import importlib.util
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

from fiducials_amd import _lib, camera  # noqa: E402
from fiducials_amd.detector import MAP_ENTRY_DTYPE, ArucoDetector  # noqa: E402

_spec = importlib.util.spec_from_file_location("gpu_map_build_bench", os.path.join(ROOT, "tools", "gpu_map_build_bench.py"))
plain_bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plain_bench)

SIZES = (64, 256, 1024)
WRONG = (0, 2)


def with_wrong_ids(c, views, per_view: int):
    """per_view markers of every view relabelled as markers of the map that the view does not show (never the fixed one)."""
    rng = np.random.default_rng(20261210)
    all_ids = [int(i) for i in c["entries"]["id"]]
    fixed = set(int(i) for i in c["fixed"]["id"])
    out = []
    for corners, ids in views:
        ids = ids.copy()
        free = [p for p, i in enumerate(ids) if int(i) not in fixed]
        absent = [i for i in all_ids if i not in ids and i not in fixed]
        k = min(per_view, len(free), len(absent))
        for p, i in zip(rng.choice(free, k, replace=False), rng.choice(absent, k, replace=False)):
            ids[p] = i
        out.append((corners, ids))
    return out


def call_robust(det, c, mk, n):
    L = det._L
    opts = _lib.FidBuildOpts()
    L.fid_default_build_opts(C.byref(opts))
    opts.fiducial_len = c["fiducial_len"]
    ropts = _lib.FidBuildRobustOpts(_lib.BUILD_ROBUST_INLIER_PX, 2, 0)
    k = c["k16"]
    cam = camera.Camera(c["model"], [[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]], k[4:9])
    fx = np.ascontiguousarray(c["fixed"], dtype=MAP_ENTRY_DTYPE)
    out, rout = np.zeros(1, _lib.BUILD_OUT_DTYPE), np.zeros(1, _lib.BUILD_ROBUST_OUT_DTYPE)
    mout = np.zeros(256, _lib.BUILD_MARKER_DTYPE)
    n_m = C.c_int32(0)
    t0 = time.perf_counter()
    rc = L.fid_build_map_robust_cam(det._ctx, C.byref(cam.c), mk.ctypes.data, n.ctypes.data, len(n), plain_bench.PER_VIEW, fx.ctypes.data, len(fx), C.byref(opts),
                                    C.byref(ropts), out.ctypes.data, rout.ctypes.data, mout.ctypes.data, len(mout), C.byref(n_m), None, None, None, None, None)
    t1 = time.perf_counter()
    assert rc == _lib.FID_OK, L.fid_last_error(det._ctx)
    return (t1 - t0) * 1e3, out[0], rout[0]


def rows_of():
    for n_markers in plain_bench.MAPS:
        c = plain_bench.views_of(n_markers)
        for wrong in WRONG:
            for size in SIZES:
                views = c["views"] * (size // 64)
                yield n_markers, wrong, size, c, plain_bench.pack(with_wrong_ids(c, views, wrong) if wrong else views)


def one_call_per_row():
    det = ArucoDetector(dictionary=6, max_width=640, max_height=480)
    for _, _, _, c, (mk, n) in rows_of():
        call_robust(det, c, mk, n)


def kernel_shares():
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
                for key in ("k_build_place_score", "k_build_obs_err", "k_map_pose_robust", "k_build_", "k_map_pose", "k_pose"):
                    if key in name:
                        tot[key] = tot.get(key, 0.0) + ns
                        break
        s = sum(tot.values())
        return {"kernel_ns": {k: int(v) for k, v in sorted(tot.items())},
                "share_place_score": round(tot.get("k_build_place_score", 0.0) / s, 5) if s else None,
                "share_obs_err": round(tot.get("k_build_obs_err", 0.0) / s, 5) if s else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_build_robust_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    if args.child:
        return one_call_per_row()
    det = ArucoDetector(dictionary=6, max_width=640, max_height=480)
    rows = []
    for n_markers, wrong, size, c, (mk, n) in rows_of():
        tr, tp = [], []
        for rep in range(args.reps + 3):
            a, out, rout = call_robust(det, c, mk, n)
            b, pout = plain_bench.call(det, c, mk, n)
            if rep >= 3:
                tr.append(a)
                tp.append(b)
        mr, mp = statistics.median(tr), statistics.median(tp)
        rows.append({"map_markers": n_markers, "views": size, "wrong_ids_per_view": wrong, "robust_median_ms": round(mr, 4), "plain_median_ms": round(mp, 4),
                     "ratio": round(mr / mp, 3), "rounds": int(rout["rounds"]), "stable": int(rout["stable"]), "outliers": int(rout["n_outliers"]),
                     "robust_trials_last_round": int(out["n_iter"]), "plain_trials": int(pout["n_iter"]), "robust_rms_px": float(out["rms"]), "plain_rms_px": float(pout["rms"])})
        print(rows[-1], flush=True)
    doc = {"what": "fid_build_map_robust_cam against fid_build_map_cam on the same views, host clock around the call, median of %d; inlier_px %.1f, "
                   "min_views_place 2, default build options" % (args.reps, _lib.BUILD_ROBUST_INLIER_PX),
           "device_text_sha256": _lib.device_text_sha256(), "rows": rows, "kernel_shares": None if args.no_profile else kernel_shares()}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"kernel_shares": doc["kernel_shares"]}))


if __name__ == "__main__":
    main()
