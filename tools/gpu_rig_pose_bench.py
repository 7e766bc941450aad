#!/usr/bin/env python3
"""What the rig pose costs (run on the GPU box): fid_rig_pose_last on the frames of a detect call beside fid_map_pose_last_cam on the
same frames in the same run, each with and without its covariance.  Shapes: 64 time steps x 4 cameras x 20 markers (256 frames at
640 x 480: one rendered time step of a 5 x 4 board, repeated) and one time step of 4 cameras.  Every call launches for the whole
batch, copies its records out and returns when they are in host memory; the figure is the median of the calls by the host clock, with
p10 / p90 beside it.  After warm-up the calls alternate, so clock drift falls on all alike.  fid_map_pose_last_cam is a remembered
request, whose second call on the same frames is a copy: FID_NO_POSE_AHEAD=1 is set here, so that every call of it launches, as
every call of fid_rig_pose_last does.
Usage: python tools/gpu_rig_pose_bench.py [--out profiles/rig_pose_bench.json] [--calls 60]"""
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
from fiducials_amd.camera import Camera, RigCamera  # noqa: E402
from fiducials_amd.detector import MAP_POSE_COV_DTYPE, MAP_POSE_DTYPE, RIG_POSE_DTYPE, ArucoDetector, map_entries  # noqa: E402
from fiducials_amd.dictionary import get_predefined_dictionary  # noqa: E402

W, H = 640, 480
K = np.array([[466.7, 0, 320.0], [0, 466.7, 240.0], [0, 0, 1.0]])
FACING = np.diag([1.0, -1.0, -1.0])
DICT, LEN, PITCH, COLS, ROWS = 6, 0.05, 0.075, 5, 4
CAMERAS = 4


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64)) * 1e6
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(ts[len(ts) // 10]), 2), "p90_us": round(float(ts[(9 * len(ts)) // 10]), 2),
            "calls": len(ts)}


def quat(rvec):
    r = np.asarray(rvec, float)
    th = np.linalg.norm(r)
    return np.concatenate([np.sin(th / 2) * r / th, [np.cos(th / 2)]])


def rig():
    """four cameras on a 6 cm square, each turned a little towards the middle"""
    cam = Camera(_lib.CAM_PLUMB_BOB, K, np.zeros(5))
    return [RigCamera.from_tf((0.03 * sx, 0.03 * sy, 0.0), quat((0.04 * sy, -0.04 * sx, 0.001)), cam) for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1))]


def board():
    k = np.arange(COLS * ROWS)
    t = np.stack([(k % COLS - (COLS - 1) / 2) * PITCH, (k // COLS - (ROWS - 1) / 2) * PITCH, np.zeros(len(k))], axis=1)
    return map_entries(k, LEN, np.broadcast_to(np.eye(3), (len(k), 3, 3)), t)


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


def shape(steps, step_frames, entries, cams, calls):
    F = steps * CAMERAS
    frames = np.ascontiguousarray(np.stack([step_frames[f % CAMERAS] for f in range(F)]))
    det = ArucoDetector(DICT, max_width=W, max_height=H, max_batch=F, max_markers=32)
    det.set_map(entries)
    det.set_rig(cams)
    found = [len(r[1]) for r in det.detect_markers_batch(frames)]
    L, ctx = det._L, det._ctx
    rig_out, rig_cov = np.zeros(steps, RIG_POSE_DTYPE), np.zeros(steps, MAP_POSE_COV_DTYPE)
    map_out, map_cov = np.zeros(F, MAP_POSE_DTYPE), np.zeros(F, MAP_POSE_COV_DTYPE)
    cam = cams[0].camera
    res = time_calls({
        "fid_rig_pose_last": lambda: L.fid_rig_pose_last(ctx, rig_out.ctypes.data, steps, 0.0, None),
        "fid_rig_pose_last, covariance": lambda: L.fid_rig_pose_last(ctx, rig_out.ctypes.data, steps, 1.0, rig_cov.ctypes.data),
        "fid_map_pose_last_cam": lambda: L.fid_map_pose_last_cam(ctx, C.byref(cam.c), map_out.ctypes.data, F),
        "fid_map_pose_last_cov_cam": lambda: L.fid_map_pose_last_cov_cam(ctx, C.byref(cam.c), map_out.ctypes.data, F, 1.0, map_cov.ctypes.data),
    }, calls)
    det.close()
    return {"time_steps": steps, "frames": F, "markers_found_per_frame": [min(found), max(found)],
            "markers_used_per_step": [int(rig_out["n_markers"].min()), int(rig_out["n_markers"].max())],
            "markers_used_per_frame_by_map_pose": [int(map_out["n_markers"].min()), int(map_out["n_markers"].max())], **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_pose_bench.json"))
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    assert a.calls >= 30
    entries, cams = board(), rig()
    R = synth._rodrigues(np.array([0.15, -0.1, 0.05])) @ FACING
    t = np.array([0.0, 0.0, 0.5])
    step_frames = [f.image for f in synth.make_rig_frames(get_predefined_dictionary(DICT), entries["id"], [(LEN, e["R"], e["t"]) for e in entries], K,
                                                          [(c.R, c.t) for c in cams], R, t, seed=5, width=W, height=H)]
    doc = {"device_text_sha256": _lib.device_text_sha256(),
           "what": "host clock around the call (one launch for the whole batch + copy + synchronise), the calls alternating; median of the calls; "
                   "FID_NO_POSE_AHEAD=1 so that fid_map_pose_last* launches on every call",
           "64 time steps x 4 cameras x 20 markers, 640 x 480": shape(64, step_frames, entries, cams, a.calls),
           "1 time step x 4 cameras x 20 markers, 640 x 480": shape(1, step_frames, entries, cams, a.calls)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
