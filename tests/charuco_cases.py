"""The boards, poses, rendered frames and hand-made marker lists the ChArUco tests share (tests/test_charuco_restatement.py on the CPU,
tests/test_gpu_charuco.py on the device): made once per process, never changed."""
from __future__ import annotations

import functools

import numpy as np

from fiducials_amd import synth
from fiducials_amd.charuco import CharucoBoard
from fiducials_amd.dictionary import get_predefined_dictionary
from stag_bundle_cases import D_NONZERO, K, exact_minimiser, project  # noqa: F401  (the same camera and minimiser as the map tests)

import charuco_restatement as cr

W, H = 640, 480
DICT = 7  # DICT_5X5_1000: the 22 x 23 board needs 253 ids
NOISE_PX = 0.3
FACING = np.diag([1.0, -1.0, -1.0])  # a board (x right, y up, z out of its face) that looks straight into the camera

# (squares_x, squares_y, square_len, marker_len, first_id)
BOARDS = {
    "5x4": (5, 4, 0.04, 0.024, 0),
    "5x4_id40": (5, 4, 0.04, 0.024, 40),
    "5x4_dyadic": (5, 4, 0.03125, 0.01953125, 0),  # lengths exact in float: as_map_entries() gives the board's own object points
    "10x9": (10, 9, 0.03125, 0.01953125, 100),     # 72 corners, 45 markers: more than one pass of 64 lanes
    "22x23": (22, 23, 0.03125, 0.01953125, 0),     # 462 corners, 253 markers: the limits
}


@functools.lru_cache(maxsize=None)
def board(name: str) -> CharucoBoard:
    return CharucoBoard(*BOARDS[name])


@functools.lru_cache(maxsize=None)
def rboard(name: str) -> cr.Board:
    return cr.Board(*BOARDS[name])


def dictionary():
    return get_predefined_dictionary(DICT)


def board_pose(name: str, tilt, dist: float, roll: float = 0.0, shift=(0.0, 0.0)):
    """The pose (R, t) of the board in the camera: the board's centre on the optical axis (moved by `shift` metres in the image plane) at
    `dist`, tilted by the rotation vector `tilt` and rolled about the axis."""
    b = board(name)
    R = synth._rodrigues(np.asarray(tilt, float)) @ synth._rodrigues(np.array([0.0, 0.0, roll])) @ FACING
    centre = np.array([b.squares_x * b.square_len / 2, b.squares_y * b.square_len / 2, 0.0])
    return R, np.array([shift[0], shift[1], dist]) - R @ centre


# ---- rendered views of the 5 x 4 board (640 x 480, square 0.04, marker 0.024)
VIEWS = {
    "frontal": ((0.0, 0.0, 0.0), 0.36, 0.0),
    "tilted": ((0.45, -0.3, 0.0), 0.40, 0.25),
    "far": ((0.1, 0.2, 0.0), 0.46, -0.4),
    "side": ((-0.3, 0.35, 0.0), 0.40, 1.2),
}


@functools.lru_cache(maxsize=None)
def view(name: str, board_name: str = "5x4", hidden: tuple = (), distorted: bool = False) -> synth.CharucoFrame:
    tilt, dist, roll = VIEWS[name]
    R, t = board_pose(board_name, tilt, dist, roll)
    fr = synth.make_charuco_frame(dictionary(), board(board_name), K, R, t, seed=sorted(VIEWS).index(name) + 11, width=W, height=H,
                                  D=D_NONZERO * 4 if distorted else None, hidden=hidden)
    fr.image.setflags(write=False)
    return fr


# ---- hand-made marker lists: exact projections of the board's marker corners plus +-0.3 px of seeded noise, as float32
def hand_markers(board_name: str, R, t, seed: int, D=None, keep=None):
    """-> (ids int32 (n,), corners float32 (n, 4, 2)) in marker order; keep: the marker indices to list (default all)"""
    b = board(board_name)
    rng = np.random.default_rng(seed)
    img = project(b.marker_object_points.reshape(-1, 3), R, t, K, np.zeros(5) if D is None else D).reshape(-1, 4, 2)
    img = (img + rng.uniform(-NOISE_PX, NOISE_PX, img.shape)).astype(np.float32)
    keep = list(range(b.n_markers)) if keep is None else list(keep)
    return b.ids[keep].astype(np.int32), img[keep]


@functools.lru_cache(maxsize=None)
def flat_gray() -> np.ndarray:
    g = np.full((H, W), 128, np.uint8)
    g.setflags(write=False)
    return g


def ulps(got, want) -> np.ndarray:
    """|got - want| in units of want's float spacing"""
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float32).astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
