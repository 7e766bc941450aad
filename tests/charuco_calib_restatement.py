"""fid_calibrate_charuco (include/fid_abi.h: "camera calibration from ChArUco corners") restated in NumPy, float64: which records of a
view are used, which views are used, and the call -- calib_restatement's AUTO start, Problem, lm and std_dev on plain (object points,
image points) lists, the object points from charuco_restatement's board.  It is the reference of tests/test_gpu_charuco_calibrate.py; no
test functions and no GPU here.

A view is a record array with the fields id, x, y (what charuco_last returns), or a pair (ids (n,), xy (n, 2))."""
from __future__ import annotations

import numpy as np

import calib_restatement as cr
import charuco_restatement as chr_

VIEW_USED, VIEW_FEW, VIEW_NO_START = 0, 1, 2
MIN_POINTS = 4


def view_records(view):
    """-> (ids int64 (n,), xy float64 (n, 2)): the records as listed, the positions float32 widened."""
    if isinstance(view, np.ndarray) and view.dtype.names and "id" in view.dtype.names:
        ids, xy = view["id"], np.stack([view["x"], view["y"]], axis=1) if len(view) else np.zeros((0, 2))
    else:
        ids, xy = view
    ids = np.asarray(ids, np.int64).reshape(-1)
    return ids, np.asarray(xy, np.float32).astype(np.float64).reshape(len(ids), 2)


def select(board: chr_.Board, view):
    """The list positions of the used records, in list order: an id that occurs more than once is left out altogether.  An id outside
    the board or a position that is not finite in any listed record is the call's refusal: ValueError."""
    ids, xy = view_records(view)
    if ((ids < 0) | (ids >= board.n_corners)).any():
        raise ValueError("a corner id outside the board")
    if not np.isfinite(xy).all():
        raise ValueError("a coordinate that is not finite")
    count = np.bincount(ids, minlength=board.n_corners)
    return [m for m, i in enumerate(ids) if count[i] == 1]


def view_points(board: chr_.Board, view):
    """-> (object points (n, 3), image points (n, 2), the used ids) of one view."""
    ids, xy = view_records(view)
    pos = select(board, view)
    return board.corner_obj[ids[pos]].reshape(-1, 3), xy[pos].reshape(-1, 2), ids[pos]


def on_one_line(board: chr_.Board, ids) -> bool:
    """exactly, on the integer (cx, cy): every point's offset from the first is parallel to the first offset that is not zero"""
    g = board.grid[np.asarray(ids, np.int64)]
    d = g - g[0]
    nz = [v for v in d if v[0] != 0 or v[1] != 0]
    return not nz or all(int(nz[0][0]) * int(v[1]) - int(nz[0][1]) * int(v[0]) == 0 for v in d)


def view_status(board: chr_.Board, view, min_points: int = MIN_POINTS) -> int:
    """What the selection alone decides (a start pose that cannot be computed for another reason is the device's to report)."""
    _, _, ids = view_points(board, view)
    if len(ids) < max(min_points, MIN_POINTS):
        return VIEW_FEW
    return VIEW_NO_START if on_one_line(board, ids) else VIEW_USED


def calibrate(board: chr_.Board, views, image_size, model: int, k16, free_mask: int, fix_aspect: bool = False, start: str = "auto",
              min_points: int = MIN_POINTS, start_poses=None):
    """The reference answer of one call -> calib_restatement.calibrate's dict, with statuses (per view) and n_used (per view) added.
    start = "auto", or "given" with start_poses (one per USED view; None: the AUTO poses under the given camera)."""
    pts_all = [view_points(board, v) for v in views]
    statuses = [view_status(board, v, min_points) for v in views]
    used = [i for i, s in enumerate(statuses) if s == VIEW_USED]
    points = [(pts_all[i][0], pts_all[i][1]) for i in used]
    if start == "auto":
        k0, poses0 = cr.auto_start(model, k16, free_mask, fix_aspect, points, image_size)
    else:
        k0 = np.asarray(k16, dtype=np.float64).copy()
        poses0 = start_poses if start_poses is not None else cr.auto_start(model, k0, 0, False, points, image_size)[1]
    prob = cr.Problem(model, k0, free_mask, fix_aspect)
    if fix_aspect:
        prob.aspect = float(k16[0]) / float(k16[1])
    x, c, it = cr.lm(prob, prob.pack(prob.k16(prob.pack(k0, [])), poses0), points)
    sd, rms = cr.std_dev(prob, x, points)
    k, poses = prob.unpack(x)
    return dict(k16=k, poses=poses, cost=c, rms=rms, std_dev=sd, used=used, n_points=sum(len(o) for o, _ in points), iterations=it, problem=prob,
                points=points, x=x, statuses=statuses, n_used=[len(p[2]) for p in pts_all])
