"""Views for the calibration tests (tests/test_calib_restatement.py on the CPU, tests/test_gpu_calibrate.py on the device): a planar
aruco_map_cases.grid_board seen under tilts of 5 - 50 degrees about random in-plane axes, every corner at least 3 px inside a 1280 x
720 frame, Gaussian noise of sigma px added, corners rounded to float32.  Made once per process, never changed.

THE KEEP RULE.  A case is a parity case only if the reference (calib_restatement.calibrate) reaches the same minimum from two starts,
the AUTO start and the generating values: relative cost gap <= KEEP_GAP.  Every case in CASES passes it (test_calib_restatement.py
asserts that; none is dropped silently).  Left out of CASES on purpose: the rational model with all eight coefficients free -- from
the two starts it ends 3e-3 apart in cost with coefficients in the tens (the issue's prototype) -- which test_gpu_calibrate.py uses
only for "runs, cost does not rise" (RATIONAL8).

MEASURED ON THE DEVICE (MI355X), the largest over CASES: see DEVICE_MEASURED below."""
from __future__ import annotations

import functools

import numpy as np

import calib_restatement as cr
import camera_model_cases as cmc
import pose_cases as pc
from aruco_map_cases import FACING, grid_board, object_points

W, H = 1280, 720
FX, FY, CX, CY = 910.0, 905.0, 652.3, 348.9
SIGMA = 0.3
KEEP_GAP = 1e-8
MARGIN = 3.0
# free masks (fid_abi.h FID_CALIB_FREE_*)
FREE_PLUMB_BOB, FREE_EQUIDISTANT = 0x01FF, 0x00FF
FREE_RATIONAL_K1_K2_K4 = 0x000F | 1 << 4 | 1 << 5 | 1 << 9
FREE_RATIONAL8 = 0x0FFF
# the largest figures measured on the MI355X over CASES (test_gpu_calibrate.py prints them): the device's cost above the reference
# minimum, relative; the parameter distance in units of the bar; std_dev and rms against the reference, relative
DEVICE_MEASURED = ("cost excess <= 3.9e-10 (noise-free cases, bar 1e-9; 1.4e-13 on the noisy ones), parameters <= 0.012 % of their bar, rms <= 8.6e-11, "
                   "std_dev <= 1.2e-7 (rational_k124 5x20_exact; 1.7e-8 outside the rational model), bars 1e-6")

# name: (model, D of the generating camera, free mask)
MODELS = {
    "plumb_bob": (cmc.PLUMB_BOB, pc.DISTORTIONS["barrel"], FREE_PLUMB_BOB),
    "equidistant": (cmc.EQUIDISTANT, cmc.SETS["fe_kb"][1], FREE_EQUIDISTANT),
    "rational_k124": (cmc.RATIONAL, (0.12, -0.05, 0.0, 0.0, 0.0, 0.03, 0.0, 0.0), FREE_RATIONAL_K1_K2_K4),
}
# (views, markers per view, columns of the board's grid, sigma)
SHAPES = {"3x6": (3, 6, 3, SIGMA), "17x1": (17, 1, 1, SIGMA), "12x12": (12, 12, 4, SIGMA), "5x20_exact": (5, 20, 5, 0.0)}
CASES = [(m, s) for m in MODELS for s in SHAPES]
RATIONAL8 = ("rational8", "12x12")
# the 16-view case whose copies make the large calls (64, 256 and 1 024 views); held to the keep rule like the others
SHAPES_LARGE = {"16x8": (16, 8, 4, SIGMA)}
LARGE_BASE = ("plumb_bob", "16x8")
# views of one 300-marker board with 64, 65, 256 and 257 markers in the list (the chunk of 64 rows, FID_MAP_MAX_USED and one over it)
SIZES = (64, 65, 256, 257)


def k16_of(D) -> np.ndarray:
    k = np.zeros(16)
    k[:4] = FX, FY, CX, CY
    k[4:4 + len(D)] = D
    return k


def _model(name: str):
    if name == "rational8":
        return cmc.RATIONAL, cmc.SETS["kinect"][1], FREE_RATIONAL8
    return MODELS[name]


@functools.lru_cache(maxsize=None)
def board(n: int, cols: int):
    e = grid_board(n, cols)
    e.setflags(write=False)
    return e


def view_pose(rng, model, k16, P):
    """A pose of the board in the camera with every corner at least MARGIN px inside the frame: tilt 5 - 50 degrees about a random
    in-plane axis, any roll, the board's centre somewhere in the frame, at a distance that makes it span 25 - 85 % of the height."""
    centre = P.mean(axis=0)
    span = float(np.linalg.norm(P.max(axis=0) - P.min(axis=0)))
    K = np.array([[k16[0], 0, k16[2]], [0, k16[1], k16[3]], [0, 0, 1.0]])
    while True:
        tilt, axis, roll = np.deg2rad(rng.uniform(5.0, 50.0)), rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-np.pi, np.pi)
        R = pc.rodrigues(np.array([np.cos(axis), np.sin(axis), 0.0]) * tilt) @ pc.rodrigues([0.0, 0.0, roll]) @ FACING
        z = k16[1] * span / (rng.uniform(0.25, 0.85) * H)
        u, v = rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.2 * H, 0.8 * H)
        nx, ny = cmc.undistort_exact(model, list(k16[4:]), (u - k16[2]) / k16[0], (v - k16[3]) / k16[1])
        t = np.array([nx * z, ny * z, z]) - R @ centre
        pcam = P @ R.T + t
        if (pcam[:, 2] < 0.05).any():
            continue
        uv = cmc.project(model, K, list(k16[4:]), R, t, P)
        if (uv[:, 0] >= MARGIN).all() and (uv[:, 0] <= W - 1 - MARGIN).all() and (uv[:, 1] >= MARGIN).all() and (uv[:, 1] <= H - 1 - MARGIN).all():
            return R, t, uv


@functools.lru_cache(maxsize=None)
def case(model_name: str, shape: str):
    """-> dict(model, k16 (generating), free, entries, views [(corners (n, 4, 2) float32, ids)], poses [(rvec, tvec) generating], image_size)."""
    model, D, free = _model(model_name)
    nv, nm, cols, sigma = {**SHAPES, **SHAPES_LARGE}[shape]
    k16 = k16_of(D)
    rng = np.random.default_rng([20261020, list({**SHAPES, **SHAPES_LARGE}).index(shape), sum(map(ord, model_name))])
    entries = board(20 if nm == 1 else nm, 5 if nm == 1 else cols)  # (one marker a view: a different marker of a 20-marker board each time)
    views, poses = [], []
    for v in range(nv):
        e = entries[[v % len(entries)]] if nm == 1 else entries
        P = object_points(e)
        R, t, uv = view_pose(rng, model, k16, P)
        uv = uv + sigma * rng.standard_normal(uv.shape)
        views.append((uv.astype(np.float32).reshape(-1, 4, 2), e["id"].astype(np.int32).copy()))
        poses.append(np.concatenate([cr.rotation_vector(R), t]))
    return dict(model=model, n_dist=len(D), k16=k16, free=free, entries=entries, views=views, poses=poses, image_size=(W, H), sigma=sigma)


@functools.lru_cache(maxsize=None)
def reference(model_name: str, shape: str):
    """The reference's answer from the two starts -> dict(auto, given, gap (relative cost gap), gap_std, gap_rms, kept)."""
    return reference_of(case(model_name, shape))


@functools.lru_cache(maxsize=None)
def sizes_case():
    """Four noise-free-plus-noise views of a 300-marker board (20 columns, 0.02 m markers) with SIZES markers in their lists."""
    model, D, free = MODELS["plumb_bob"]
    k16 = k16_of(D)
    entries = grid_board(300, 20, length=0.02, pitch=0.03)
    entries.setflags(write=False)
    rng = np.random.default_rng(20261021)
    views, poses = [], []
    for n in SIZES:
        P = object_points(entries)
        R, t, uv = view_pose(rng, model, k16, P)
        uv = (uv + SIGMA * rng.standard_normal(uv.shape)).astype(np.float32).reshape(-1, 4, 2)
        views.append((uv[:n].copy(), entries["id"][:n].astype(np.int32).copy()))
        poses.append(np.concatenate([cr.rotation_vector(R), t]))
    return dict(model=model, n_dist=len(D), k16=k16, free=free, entries=entries, views=views, poses=poses, image_size=(W, H), sigma=SIGMA)


@functools.lru_cache(maxsize=None)
def sizes_reference():
    c = sizes_case()
    # (the reference takes what the device takes: the first FID_MAP_MAX_USED markers of a list; the generating poses are all views')
    return reference_of(c)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """plumb_bob 12x12's board and first six views, disturbed: view 1 holds only ids the map lacks, view 2 has two mapped markers (below
    min_markers = 3), view 3 shows id 5 twice (both out), view 4 has unmapped ids among its markers."""
    base = case("plumb_bob", "12x12")
    views = [(c.copy(), i.copy()) for c, i in base["views"][:6]]
    views[1] = (views[1][0], views[1][1] + 500)
    views[2] = (views[2][0][:2].copy(), views[2][1][:2].copy())
    c3, i3 = views[3]
    views[3] = (np.concatenate([c3, c3[5:6] + 40.0]), np.concatenate([i3, i3[5:6]]))
    c4, i4 = views[4]
    views[4] = (np.concatenate([c4[:4], c4[:3] + 7.0, c4[4:]]), np.concatenate([i4[:4], np.array([700, 701, 702], np.int32), i4[4:]]))
    return dict(base, views=views, poses=None, min_markers=3)


@functools.lru_cache(maxsize=None)
def mixed_reference():
    return reference_of(mixed_case(), min_markers=3)


def reference_of(c, min_markers: int = 1):
    a = cr.calibrate(c["entries"], c["views"], c["image_size"], c["model"], zero_start(c), c["free"], start="auto", min_markers=min_markers)
    if c.get("poses") is None:  # (no generating poses at hand for the used views: the second start is the AUTO poses under the generating camera)
        g = cr.calibrate(c["entries"], c["views"], c["image_size"], c["model"], c["k16"], c["free"], start="given", min_markers=min_markers)
    else:
        g = _given(c, min_markers)
    return _compare(c, a, g)


def _given(c, min_markers):
    return cr.calibrate(c["entries"], c["views"], c["image_size"], c["model"], c["k16"], c["free"], start="given", start_poses=c["poses"],
                        min_markers=min_markers)


def _compare(c, a, g):
    gap = abs(a["cost"] - g["cost"]) / min(a["cost"], g["cost"])
    free = [i for i in range(16) if c["free"] >> i & 1]
    gap_std = float(np.max(np.abs(a["std_dev"][free] - g["std_dev"][free]) / g["std_dev"][free]))
    gap_rms = abs(a["rms"] - g["rms"]) / g["rms"]
    best = a if a["cost"] <= g["cost"] else g
    return dict(auto=a, given=g, best=best, gap=gap, gap_std=gap_std, gap_rms=gap_rms, kept=gap <= KEEP_GAP)


def zero_start(c) -> np.ndarray:
    """What a caller hands to the AUTO start: the fixed slots' values, everything free at a placeholder."""
    k = c["k16"].copy()
    for i in range(16):
        if c["free"] >> i & 1:
            k[i] = 1.0 if i < 2 else 0.0
    return k
