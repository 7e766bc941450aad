"""The rigs, maps and hand-made marker sets the rig pose tests share (tests/test_rig_restatement.py on the CPU,
tests/test_gpu_rig_pose*.py on the device): made once per process, never changed.  No test functions and no GPU.

A case is a rig (rig_restatement.Cam per camera), a map, the pose of the map in the RIG frame, and per camera the ids and corners
(float32) that camera hands in: every marker of the map projected through rig pose, extrinsic and the camera's own model, exact or
with +-0.3 px uniform noise, the list cut per camera as the case says."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import aruco_map_cases as mc
import camera_model_cases as cm
import rig_restatement as rr
from fiducials_amd import synth
from fiducials_amd.camera import Camera, RigCamera

W, H = mc.W, mc.H
K = mc.K
NOISE_PX = mc.NOISE_PX
MODELS = {
    "pb": (cm.PLUMB_BOB, tuple(mc.D_NONZERO)),
    "rat": cm.SETS["prism12"],
    "fe": cm.SETS["fe_kb"],
}


def _quat(rvec):
    r = np.asarray(rvec, float)
    th = np.linalg.norm(r)
    return np.concatenate([np.sin(th / 2) * r / th, [np.cos(th / 2)]]) if th > 0 else np.array([0.0, 0.0, 0.0, 1.0])


def make_cam(model_name: str, xyz, rvec) -> rr.Cam:
    """A camera at xyz in the rig frame, turned by rvec from the rig's axes (the rig looks along its z, like a camera)."""
    model, D = MODELS[model_name]
    R, t = rr.from_tf(xyz, _quat(rvec))
    return rr.Cam(model, K, tuple(D), R, t)


def lib_rig(cams):
    """rig_restatement.Cam -> fiducials_amd.camera.RigCamera, what ArucoDetector.set_rig takes."""
    return [RigCamera(Camera(c.model, c.K, c.D), c.R, c.t) for c in cams]


# two and three cameras a few centimetres apart with converging axes; all three models in the second
RIG2 = (make_cam("pb", (-0.06, 0.0, 0.0), (0.0, 0.08, 0.0)), make_cam("rat", (0.06, 0.01, 0.0), (0.0, -0.08, 0.02)))
RIG3 = (make_cam("pb", (-0.1, 0.0, 0.0), (0.0, 0.1, 0.0)), make_cam("fe", (0.0, 0.03, 0.01), (0.02, 0.0, 0.0)), make_cam("rat", (0.1, 0.0, 0.0), (0.01, -0.1, 0.0)))
RIG1_IDENTITY = (rr.Cam(cm.PLUMB_BOB, K, tuple(mc.D_NONZERO), np.eye(3), np.zeros(3)),)
RIG1_MOVED = (make_cam("pb", (0.05, -0.02, 0.03), (0.1, -0.2, 0.05)),)


@dataclass(frozen=True)
class Case:
    name: str
    cams: tuple
    entries: np.ndarray
    R: np.ndarray        # the map in the rig frame
    t: np.ndarray
    ids: tuple           # per camera: (n_c,) int32
    corners: tuple       # per camera: (n_c, 4, 2) float32
    noisy: bool


def observe(cams, entries, R, t, keep, noise_rng=None):
    """Per camera c the markers keep[c] (indices into entries) projected through the rig: (ids, corners float32)."""
    ids, corners = [], []
    for c, cam in enumerate(cams):
        e = entries[list(keep[c])]
        if len(e) == 0:
            ids.append(np.zeros(0, np.int32))
            corners.append(np.zeros((0, 4, 2), np.float32))
            continue
        img = cm.project(cam.model, cam.K, cam.D, cam.R @ R, cam.R @ t + cam.t, mc.object_points(e))
        assert (img[:, 0] > 2).all() and (img[:, 0] < W - 2).all() and (img[:, 1] > 2).all() and (img[:, 1] < H - 2).all(), "a marker outside the frame"
        if noise_rng is not None:
            img = img + noise_rng.uniform(-NOISE_PX, NOISE_PX, img.shape)
        ids.append(e["id"].astype(np.int32))
        corners.append(mc.split_markers(img))
    return tuple(ids), tuple(corners)


def _board(n, cols, oblique=False, small=False):
    Rb = mc.OBLIQUE if oblique else np.eye(3)
    kw = dict(length=0.0625, pitch=0.09375) if small else {}
    e = mc.grid_board(n, cols, Rb, np.zeros(3), first_id=40, **kw)
    return e, Rb


# (name, rig, markers of the board, its columns, small markers, per camera the board's markers it sees)
LAYOUTS = (
    ("one_marker_one_camera", RIG2, 4, 2, False, ((2,), ())),
    ("two_cameras_one_marker_each", RIG2, 4, 2, False, ((1,), (2,))),
    ("two_cameras", RIG2, 6, 3, False, ((0, 1, 2, 3, 4, 5), (5, 3, 1, 0))),
    ("three_models", RIG3, 6, 3, False, ((0, 1, 3, 4), (0, 1, 2, 3, 4, 5), (1, 2, 4, 5))),
    ("seventeen", RIG3, 6, 3, False, ((0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 4))),
    ("middle_camera_blind", RIG3, 6, 3, False, ((0, 1, 3), (), (2, 4, 5))),
    ("three_over", RIG3, 44, 11, True, (tuple(range(44)), tuple(range(44)), tuple(range(43)))),
)


@functools.lru_cache(maxsize=None)
def cases():
    """Every layout with exact and with noisy projections, the board flat and oblique in the map by turns."""
    out = []
    rng = np.random.default_rng(20261021)
    for i, (name, cams, n, cols, small, keep) in enumerate(LAYOUTS):
        e, Rb = _board(n, cols, oblique=bool(i & 1), small=small)
        e.setflags(write=False)
        R, t = mc.board_pose(rng, Rb, np.zeros(3), tz_range=(1.0, 1.3), tilt_deg=(10.0, 25.0))
        t = np.array([0.02, -0.01, t[2]])  # (in front of the rig, so that every camera has the whole board in its frame)
        for noisy in (False, True):
            ids, corners = observe(cams, e, R, t, keep, rng if noisy else None)
            out.append(Case(name + ("_noisy" if noisy else ""), cams, e, R, t, ids, corners, noisy))
    return tuple(out)


def case(name: str) -> Case:
    return [c for c in cases() if c.name == name][0]


@functools.lru_cache(maxsize=None)
def restated(name: str, sigma_px=None) -> dict:
    """rig_restatement.restate on a case, once per process."""
    c = case(name)
    return rr.restate(c.cams, c.entries, c.ids, c.corners, sigma_px)


@functools.lru_cache(maxsize=None)
def gap_to_minimum() -> float:
    """The largest distance between the RESTATEMENT and the exact minimiser of the same joint reprojection error (Gauss-Newton from
    the truth to a step below 1e-14) over the noisy cases: what CvLevMarq's stop rule (20 steps / FLT_EPSILON) leaves."""
    worst = 0.0
    for c in cases():
        if c.noisy:
            r = restated(c.name)
            pm = rr.exact_minimum(c.cams, r["pcam"], r["P"], r["img"], np.concatenate([rr.rotvec(c.R), c.t]))
            worst = max(worst, dist(r["R"], r["tvec"], rr.rodrigues(pm[:3]), pm[3:]))
    return worst


def dist(Ra, ta, Rb, tb) -> float:
    return float(max(np.abs(np.asarray(Ra) - Rb).max(), np.abs(np.asarray(ta) - tb).max()))


# ---- the start camera: two identical cameras at mirrored extrinsics looking at a board that is its own mirror image
def mirrored_tie():
    """(cams, entries, ids, corners): camera 1 is camera 0 mirrored in the rig's plane x = 0, the board is symmetric in it, camera
    0's corners are rounded to 1 / 8 px and camera 1's ARE their mirror images (u -> 640 - u with cx = 320, the marker and the corner
    order swapped as the mirror swaps them), so that the two summed areas are equal bit for bit: shoelace terms of multiples of
    1 / 8 below 640 are exact in double in any order."""
    cam0 = rr.Cam(cm.PLUMB_BOB, K, (), *rr.from_tf((-0.08, 0.0, 0.0), _quat((0.0, 0.1, 0.0))))
    cam1 = rr.Cam(cm.PLUMB_BOB, K, (), *rr.from_tf((0.08, 0.0, 0.0), _quat((0.0, -0.1, 0.0))))
    assert K[0, 2] == W / 2
    e = mc.grid_board(4, 2, np.eye(3), np.zeros(3), first_id=60)
    R, t = mc.FACING, np.array([0.0, 0.02, 1.0])
    (ids0, _), (c0, _) = observe((cam0, cam1), e, R, t, ((0, 1, 2, 3), ()))
    c0 = (np.round(c0.astype(np.float64) * 8) / 8).astype(np.float32)
    partner = {0: 1, 1: 0, 2: 3, 3: 2}  # the marker on the other side of the plane x = 0
    c1 = np.zeros_like(c0)
    for k in range(4):
        m = c0[k][[1, 0, 3, 2]].copy()
        m[:, 0] = W - m[:, 0]
        c1[partner[k]] = m
    return (cam0, cam1), e, (ids0, ids0.copy()), (c0, c1)


# ---- a rendered scene: two cameras 12 cm apart with converging axes, a 3 x 2 board
SCENE_RIG = (rr.Cam(cm.PLUMB_BOB, K, (), *rr.from_tf((-0.06, 0.0, 0.0), _quat((0.0, 0.09, 0.0)))),
             rr.Cam(cm.PLUMB_BOB, K, (), *rr.from_tf((0.06, 0.0, 0.0), _quat((0.0, -0.09, 0.0)))))


def scene_pose():
    return synth._rodrigues(np.array([0.25, 0.15, 0.0])) @ synth._rodrigues(np.array([0.0, 0.0, 0.1])) @ mc.FACING, np.array([0.0, -0.01, 0.66])


@functools.lru_cache(maxsize=None)
def scene_frames():
    """synth.make_rig_frames on the 3 x 2 scene map: one ArucoBoardFrame per camera of SCENE_RIG."""
    from fiducials_amd.dictionary import get_predefined_dictionary

    e = mc.scene_map("3x2")
    R, t = scene_pose()
    frames = synth.make_rig_frames(get_predefined_dictionary(mc.DICT), e["id"], [(float(x["len"]), x["R"], x["t"]) for x in e], K,
                                   [(c.R, c.t) for c in SCENE_RIG], R, t, seed=11, width=W, height=H)
    for f in frames:
        f.image.setflags(write=False)
    return tuple(frames)
