"""Views for the map building tests (tests/test_map_build_restatement.py on the CPU, tests/test_gpu_map_build.py on the device):
aruco_map_cases' boards and two-wall corner seen by 640 x 480 cameras placed with look_at, the corners projected by
camera_model_cases.project, uniform noise of +-NOISE_PX added, rounded to float32.  A view lists the markers whose four corners lie
at least MARGIN px inside the frame, or the ones the case names.  Made once per process, never changed.

THE KEEP RULE (calib_cases').  A case is a parity case only if the reference (map_build_restatement.build) reaches the same minimum
from two starts, the rule's start and the generating poses: relative cost gap <= KEEP_GAP.  Every case in CASES passes it
(test_map_build_restatement.py asserts that; none is dropped silently)."""
from __future__ import annotations

import functools

import numpy as np

import camera_model_cases as cmc
import map_build_restatement as mb
import pose_cases as pc
from aruco_map_cases import H, NOISE_PX, W, corner_of_two_walls, fid_corners, grid_board, look_at
from calib_restatement import rotation_vector

FX, FY, CX, CY = 466.7, 466.7, 320.0, 240.0
KEEP_GAP = 1e-8
MARGIN = 3.0
CAMERAS = {
    "plumb_bob": (cmc.PLUMB_BOB, pc.DISTORTIONS["barrel"]),
    "rational": (cmc.RATIONAL, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004)),
    "equidistant": (cmc.EQUIDISTANT, cmc.SETS["fe_kb"][1]),
    "pinhole": (cmc.PLUMB_BOB, (0.0, 0.0, 0.0, 0.0, 0.0)),
}


def k16_of(D) -> np.ndarray:
    k = np.zeros(16)
    k[:4] = FX, FY, CX, CY
    k[4:4 + len(D)] = D
    return k


def see(entries, cam_pos, target, camera: str, rng, only=None, noise: float = NOISE_PX, min_area: float = 0.0):
    """One view -> ((corners (n, 4, 2) float32, ids int32), (rvec, tvec) generating): the markers of `only` (ids; None: all) whose
    corners are inside the frame and that face the camera."""
    model, D = CAMERAS[camera]
    k16 = k16_of(D)
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
    R, t = look_at(cam_pos, target)
    corners, ids = [], []
    for e in entries:
        if only is not None and int(e["id"]) not in only:
            continue
        P = fid_corners(e["len"]) @ e["R"].T + e["t"]
        pcam = P @ R.T + t
        if (pcam[:, 2] < 0.1).any() or (R @ e["R"][:, 2]) @ pcam.mean(axis=0) >= 0:  # behind, or seen from the back
            continue
        pin = pcam[:, :2] / pcam[:, 2:] * (FX, FY) + (CX, CY)  # (far off the axis a distortion polynomial folds back into the frame)
        if (np.abs(pin[:, 0] - CX) > 0.75 * W).any() or (np.abs(pin[:, 1] - CY) > 0.75 * H).any():
            continue
        uv = cmc.project(model, K, list(k16[4:]), R, t, P)
        if (uv[:, 0] < MARGIN).any() or (uv[:, 0] > W - 1 - MARGIN).any() or (uv[:, 1] < MARGIN).any() or (uv[:, 1] > H - 1 - MARGIN).any():
            continue
        if mb.area(uv) < min_area:  # (a marker too small or too oblique for a detector to report)
            continue
        corners.append(uv + rng.uniform(-noise, noise, size=uv.shape))
        ids.append(int(e["id"]))
    return (np.asarray(corners, np.float32).reshape(-1, 4, 2), np.asarray(ids, np.int32)), np.concatenate([rotation_vector(R), t])


def wall_views(entries, n_views: int, camera: str, seed: int, dist=(0.55, 0.9), only=None, noise: float = NOISE_PX, spread: float = 0.7, grid=None,
               tilt_deg=(12.0, 35.0), min_area: float = 0.0):
    """n_views cameras in front of a board in the plane z = 0 (its markers face +z... the map's -z side is behind them): targets spread
    over the board (grid = (nx, ny): on a grid of nx x ny cells instead), positions off the target's normal by tilt_deg degrees."""
    rng = np.random.default_rng([20261101, seed])
    lo, hi = entries["t"].min(axis=0), entries["t"].max(axis=0)
    views, poses = [], []
    for v in range(n_views):
        for _ in range(200):
            f = (v + 0.5) / n_views if grid is None else (v % grid[0] + 0.5) / grid[0]
            fy = rng.uniform(0.2, 0.8) if grid is None else (v // grid[0] + 0.5) / grid[1]
            target = np.array([lo[0] + (hi[0] - lo[0]) * (0.5 - spread / 2 + spread * f), lo[1] + (hi[1] - lo[1]) * fy, 0.0])
            d = rng.uniform(*dist)
            tilt, az = np.deg2rad(rng.uniform(*tilt_deg)), rng.uniform(0, 2 * np.pi)
            pos = target + d * np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)])
            view, pose = see(entries, pos, target, camera, rng, only=None if only is None else only[v], noise=noise, min_area=min_area)
            if len(view[1]) >= 2:
                break
        else:
            raise AssertionError("no view found")
        views.append(view)
        poses.append(pose)
    return views, poses


def _true_markers(entries):
    return {int(e["id"]): np.concatenate([rotation_vector(np.asarray(e["R"])), e["t"]]) for e in entries}


def _case(entries, views, poses, camera, fixed_ids, **kw):
    model, D = CAMERAS[camera]
    entries.setflags(write=False)
    fixed = entries[np.isin(entries["id"], fixed_ids)].copy()
    return dict(model=model, camera=camera, D=D, k16=k16_of(D), entries=entries, views=views, poses=poses, fixed=fixed, fiducial_len=float(entries["len"][0]),
                len_override=kw.pop("len_override", None), min_views=kw.pop("min_views", 2), true_markers=_true_markers(entries), **kw)


# facing the camera side z > 0: grid_board's markers have their z axis along the board's +z
def _board(n, cols, **kw):
    return grid_board(n, cols, **kw)


@functools.lru_cache(maxsize=None)
def case(name: str):
    if name.startswith("chain3"):
        # A (fixed) B C in a row; view 0: A B, view 1: B C, view 2: A B
        e = _board(3, 3)
        views, poses = wall_views(e, 3, "plumb_bob", 1, dist=(0.45, 0.6), only=[{0, 1}, {1, 2}, {0, 1}])
        return _case(e, views, poses, "plumb_bob", [0], min_views=1 if name == "chain3_min1" else 2)
    if name == "two_components":
        e = np.concatenate([_board(4, 2), _board(2, 2, tb=np.array([3.0, 0.0, 0.0]), first_id=10)])
        va, pa = wall_views(e[:4], 4, "plumb_bob", 2)
        vb, pb = wall_views(e[4:], 2, "plumb_bob", 3, dist=(0.45, 0.6))
        return _case(e, va + vb, pa + pb, "plumb_bob", [0])
    if name.startswith("size"):
        # n free markers and one fixed one: the reduced system has 6 n rows
        n = int(name[4:])
        big = n > 30
        e = _board(n + 1, 16 if big else 6 if n > 15 else 4)
        views, poses = wall_views(e, 16 if big else 6, "plumb_bob", (300 if big else 10) + n, dist=(0.9, 1.0) if big else (1.0, 1.25) if n > 15 else (0.7, 1.0),
                                  spread=1.0 if big else 0.2, grid=(8, 2) if big else None, tilt_deg=(22.0, 36.0) if big else (12.0, 35.0), min_area=600.0 if big else 0.0)
        return _case(e, views, poses, "plumb_bob", [0])
    if name == "mixed":
        # two fixed entries (0, 5), id 7 with a length of its own, id 3 twice in view 2
        e = _board(12, 4).copy()
        e["len"][7] = 0.09375
        views, poses = wall_views(e, 6, "plumb_bob", 40, dist=(0.75, 1.0))
        c2, i2 = views[2]
        at = int(np.nonzero(i2 == 3)[0][0]) if (i2 == 3).any() else 0
        views[2] = (np.concatenate([c2, c2[at:at + 1] + 25.0]), np.concatenate([i2, np.array([3 if (i2 == 3).any() else i2[0]], np.int32)]))
        return _case(e, views, poses, "plumb_bob", [0, 5], len_override={7: 0.09375, 999: 0.5})
    if name == "lists":
        # views that list 64, 65, 80 and 64 markers of an 80-marker board of small markers
        e = grid_board(80, 10, length=0.02, pitch=0.03)
        views, poses = wall_views(e, 4, "pinhole", 50, dist=(0.42, 0.5))
        for v, n in enumerate((64, 65, 80, 64)):
            c, i = views[v]
            assert len(i) >= n, (v, len(i))
            views[v] = (c[:n].copy(), i[:n].copy())
        return _case(e, views, poses, "pinhole", [0, 9, 50, 59])  # (a wide quadrilateral of fixed markers: 20 px markers alone start a view badly)
    if name.startswith("model_"):
        cam = name[6:]
        e = _board(6, 3)
        views, poses = wall_views(e, 6, cam, 60 + len(cam), dist=(0.6, 0.85))
        return _case(e, views, poses, cam, [0])
    if name == "views16":
        e = _board(8, 4)
        views, poses = wall_views(e, 16, "plumb_bob", 70, dist=(0.7, 0.95))
        return _case(e, views, poses, "plumb_bob", [0])
    if name == "corner":
        e = corner_of_two_walls(4, 4)
        rng = np.random.default_rng(20261102)
        views, poses = [], []
        for v in range(10):
            pos = np.array([rng.uniform(0.45, 0.8), rng.uniform(-0.1, 0.35), rng.uniform(0.45, 0.8)])
            view, pose = see(e, pos, np.array([0.15, 0.1, 0.15]) + rng.uniform(-0.05, 0.05, 3), "plumb_bob", rng)
            views.append(view)
            poses.append(pose)
        return _case(e, views, poses, "plumb_bob", [0])
    raise KeyError(name)


CASES = ("chain3_min1", "chain3_min2", "two_components", "size10", "size11", "size21", "size22", "mixed", "lists", "model_plumb_bob", "model_rational",
         "model_equidistant", "views16", "corner")
LARGE = "size127"   # 128 markers in the solve; 16 views
TOO_MANY = "size128"  # 129


def reference_of(c, **kw):
    args = dict(len_override=c["len_override"], min_views=c["min_views"])
    args.update(kw)
    a = mb.build(c["model"], c["k16"], c["views"], c["fixed"], c["fiducial_len"], **args)
    g = mb.build(c["model"], c["k16"], c["views"], c["fixed"], c["fiducial_len"], start_poses=(c["true_markers"], dict(enumerate(c["poses"]))), **args)
    gap = abs(a["cost"] - g["cost"]) / min(a["cost"], g["cost"])
    ids = sorted(a["cov"])
    da = np.array([np.diag(a["cov"][i]) for i in ids]).reshape(-1)
    dg = np.array([np.diag(g["cov"][i]) for i in ids]).reshape(-1)
    gap_cov = float(np.max(np.abs(da - dg) / dg)) if len(dg) else 0.0
    gap_rms = abs(a["rms"] - g["rms"]) / g["rms"]
    best = a if a["cost"] <= g["cost"] else g
    return dict(rule=a, given=g, best=best, gap=gap, gap_cov=gap_cov, gap_rms=gap_rms, kept=gap <= KEEP_GAP)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    return reference_of(case(name))
