"""The diamonds, poses, rendered frames and hand-made marker lists the diamond tests share (tests/test_diamond_restatement.py on the CPU,
tests/test_gpu_diamond.py on the device): made once per process, never changed.  At import every hand-made case is run through the
restatement and every decision of its matching is shown to have a relative margin of at least MIN_MARGIN: the device computes q_k by
another formula and may differ from the restatement by an ulp of a float pixel coordinate (6e-5 px at 640), which is 1e-5 of the
smallest tolerance used here (10.8 px) -- a hundred times less than the margin asked for."""
from __future__ import annotations

import functools

import numpy as np

from fiducials_amd import synth
from fiducials_amd.charuco import CharucoDiamond
from fiducials_amd.dictionary import get_predefined_dictionary
from stag_bundle_cases import K, project  # noqa: F401  (the same camera as the map and board tests)

import diamond_restatement as dr

W, H = 640, 480
DICT = 7  # DICT_5X5_1000
NOISE_PX = 0.3
SQUARE, MARKER = 0.04, 0.024
RATE = SQUARE / MARKER
MIN_MARGIN = 1e-3
FACING = np.diag([1.0, -1.0, -1.0])  # a sheet (x right, y up, z out of its face) that looks straight into the camera
Z5 = np.zeros(5)


def dictionary():
    return get_predefined_dictionary(DICT)


@functools.lru_cache(maxsize=None)
def diamond(ids: tuple) -> CharucoDiamond:
    return CharucoDiamond(ids, SQUARE, MARKER)


def sheet_pose(centre, tilt, dist: float, roll_deg: float = 0.0, shift_px=(0.0, 0.0)):
    """(R, t) of a sheet in the camera: the sheet point `centre` on the optical axis, moved by shift_px pixels, at `dist`, tilted by
    the rotation vector `tilt` and rolled about the axis"""
    R = synth._rodrigues(np.asarray(tilt, float)) @ synth._rodrigues(np.array([0.0, 0.0, np.deg2rad(roll_deg)])) @ FACING
    return R, np.array([shift_px[0] * dist / K[0, 0], shift_px[1] * dist / K[1, 1], dist]) - R @ np.asarray(centre, float)


def diamond_pose(tilt, dist: float, roll_deg: float = 0.0, shift_px=(0.0, 0.0)):
    return sheet_pose(diamond((0, 1, 2, 3)).centre, tilt, dist, roll_deg, shift_px)


def loose_pose(marker_len: float, tilt, dist: float, roll_deg: float, shift_px):
    return sheet_pose((0.75 * marker_len, 0.75 * marker_len, 0.0), tilt, dist, roll_deg, shift_px)


def hand_diamond(ids, R, t, rng=None):
    """-> (ids int32 (4,), corners float32 (4, 4, 2)): the exact projections of the diamond's marker corners, with +-NOISE_PX of noise
    when rng is given"""
    b = diamond(tuple(int(i) for i in ids))
    img = project(b.marker_object_points.reshape(-1, 3), R, t, K, Z5).reshape(4, 4, 2)
    if rng is not None:
        img = img + rng.uniform(-NOISE_PX, NOISE_PX, img.shape)
    return b.ids.copy(), img.astype(np.float32)


def hand_loose(marker_len: float, R, t, rng=None):
    """-> corners float32 (4, 2) of synth.make_diamond_frame's loose marker under (R, t)"""
    obj = synth._LooseMarker(0, marker_len).marker_object_points.reshape(4, 3)
    img = project(obj, R, t, K, Z5)
    if rng is not None:
        img = img + rng.uniform(-NOISE_PX, NOISE_PX, img.shape)
    return img.astype(np.float32)


def true_corners(R, t) -> np.ndarray:
    """(4, 2): the true projections of a diamond's chessboard corners in the order of fid_diamond.corners"""
    return project(diamond((0, 1, 2, 3)).record_object_points, R, t, K, Z5)


class Case:
    """A marker list with its image and what the restatement makes of it"""

    def __init__(self, name, ids, corners, image, rate=RATE, max_rep_rate=1.0, truth=None):
        self.name, self.rate, self.max_rep_rate = name, float(rate), float(max_rep_rate)
        self.ids = np.asarray(ids, np.int32).reshape(-1)
        self.corners = np.asarray(corners, np.float32).reshape(-1, 4, 2)
        self._image = image  # (a callable: the picture is rendered when a test first asks for it)
        self.truth = truth  # per expected diamond: (4, 2) true chessboard corner projections (or None)
        self.ids.setflags(write=False)
        self.corners.setflags(write=False)
        self.min_side = min(dr.side(c) for c in self.corners)
        self.want, self.margins = dr.detect(self.rate, self.max_rep_rate, self.ids, self.corners, W, H)
        assert self.margins.worst() >= MIN_MARGIN, (name, self.margins.worst())

    @property
    def image(self) -> np.ndarray:
        return self._image()


# ---- rendered frames (640 x 480): the pictures the hand-made lists are refined on, and the end-to-end inputs
ROLLS = (0.0, 90.0, 180.0, 37.0)
ONE_IDS = (5, 6, 7, 8)
# (markers of 0.024 m at 0.27 m: 41 px; the diamonds left and right, the loose markers in a column between them)
TWO = (((10, 11, 12, 13), (0.15, -0.1, 0.0), 0.27, 8.0, (-202.0, 5.0)), ((3, 3, 9, 3), (-0.1, 0.15, 0.0), 0.27, -97.0, (202.0, -5.0)))
LOOSE = ((40, MARKER, (0.2, 0.1, 0.0), 0.27, 10.0, (0.0, -180.0)), (41, MARKER, (0.0, 0.2, 0.0), 0.27, -30.0, (5.0, -62.0)),
         (42, MARKER, (-0.2, 0.0, 0.0), 0.27, 200.0, (-4.0, 60.0)), (43, MARKER, (0.1, -0.1, 0.0), 0.27, 95.0, (0.0, 180.0)))


def one_pose(roll_deg: float):
    return diamond_pose((0.25, -0.2, 0.0), 0.25, roll_deg)


@functools.lru_cache(maxsize=None)
def one_frame(roll_deg: float) -> synth.DiamondFrame:
    """one diamond, tilted, rolled by roll_deg"""
    R, t = one_pose(roll_deg)
    fr = synth.make_diamond_frame(dictionary(), [(diamond(ONE_IDS), R, t)], K, seed=31 + int(roll_deg), width=W, height=H)
    fr.image.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def frontal_frame() -> synth.DiamondFrame:
    R, t = diamond_pose((0.0, 0.0, 0.0), 0.27)
    fr = synth.make_diamond_frame(dictionary(), [(diamond(ONE_IDS), R, t)], K, seed=30, width=W, height=H)
    fr.image.setflags(write=False)
    return fr


def two_poses():
    return [diamond_pose(tilt, dist, roll, shift) for _, tilt, dist, roll, shift in TWO], [loose_pose(m, tilt, dist, roll, shift) for _, m, tilt, dist, roll, shift in LOOSE]


@functools.lru_cache(maxsize=None)
def two_frame() -> synth.DiamondFrame:
    """two diamonds (one of them with three equal ids) and four loose markers"""
    dp, lp = two_poses()
    fr = synth.make_diamond_frame(dictionary(), [(diamond(ids), R, t) for (ids, *_), (R, t) in zip(TWO, dp)], K, seed=41,
                                  loose=[(i, m, R, t) for (i, m, *_), (R, t) in zip(LOOSE, lp)], width=W, height=H)
    fr.image.setflags(write=False)
    return fr


# ---- hand-made marker lists
@functools.lru_cache(maxsize=None)
def case_one(roll_deg: float) -> Case:
    R, t = one_pose(roll_deg)
    ids, corners = hand_diamond(ONE_IDS, R, t, np.random.default_rng(100 + int(roll_deg)))
    return Case("one@%g" % roll_deg, ids, corners, lambda: one_frame(roll_deg).image, truth=[true_corners(R, t)])


def _two_lists(seed: int):
    rng = np.random.default_rng(seed)
    dp, lp = two_poses()
    ids, corners = [], []
    for (dids, *_), (R, t) in zip(TWO, dp):
        i, c = hand_diamond(dids, R, t, rng)
        ids += i.tolist()
        corners += list(c)
    for (lid, m, *_), (R, t) in zip(LOOSE, lp):
        ids.append(lid)
        corners.append(hand_loose(m, R, t, rng))
    return np.array(ids, np.int32), np.array(corners, np.float32), [true_corners(R, t) for R, t in dp]


# list order: partners and loose markers first, every anchor (layout marker 0: list entries 0 and 4 before the shuffle) after its partners
TWO_ORDER = (9, 6, 3, 1, 8, 5, 2, 10, 7, 4, 11, 0)


@functools.lru_cache(maxsize=None)
def case_two() -> Case:
    ids, corners, truth = _two_lists(7)
    o = list(TWO_ORDER)
    return Case("two shuffled", ids[o], corners[o], lambda: two_frame().image, truth=[truth[1], truth[0]])


@functools.lru_cache(maxsize=None)
def case_three_of_four() -> Case:
    c = case_one(37.0)
    return Case("three of four", c.ids[[0, 1, 3]], c.corners[[0, 1, 3]], lambda: c.image)


@functools.lru_cache(maxsize=None)
def case_equal_ids() -> Case:
    c = case_one(90.0)
    return Case("four equal ids", np.full(4, 77, np.int32), c.corners, lambda: c.image, truth=c.truth)


@functools.lru_cache(maxsize=None)
def case_margin() -> Case:
    """A noise-free diamond that faces the camera, rolled by 45 degrees and moved so that its chessboard corner 0 -- the one of its
    corners that layout marker 0, the anchor, takes part in -- lies at x = 1.8, inside the 2 px margin: not reported.  A copy of the
    anchor 0.6 px further right comes last in the list: with the first diamond's markers released it would found a diamond whose
    corner 0 lies at x = 2.1 and is selected; they stay assigned, so it founds nothing."""
    R, t = diamond_pose((0.0, 0.0, 0.0), 0.27, roll_deg=45.0)
    u = true_corners(R, t)[:, 0]  # (record corner 3 is chessboard corner 0)
    assert u.argmin() == 3 and np.sort(u)[1] - u[3] > 30
    R, t = diamond_pose((0.0, 0.0, 0.0), 0.27, roll_deg=45.0, shift_px=(1.8 - u[3], 0.0))
    ids, corners = hand_diamond((20, 21, 22, 23), R, t)
    assert abs(true_corners(R, t)[3, 0] - 1.8) < 1e-3
    ids = np.concatenate([ids, [24]]).astype(np.int32)
    corners = np.concatenate([corners, corners[:1] + np.float32([0.6, 0.0])])
    c = Case("corner in the margin", ids, corners, lambda: frontal_frame().image)
    # (what the copy alone would give: a reported diamond)
    alone, _ = dr.detect(RATE, 1.0, ids[1:], corners[1:], W, H)
    assert len(c.want) == 0 and len(alone) == 1 and alone[0]["corners0"][:, 0].min() > 2.05
    return c


def _grid(nx: int, ny: int, n: int, square_px: float, first_id: int = 0):
    """n frontal, noise-free diamonds on an nx x ny grid that fills the frame, squares of square_px pixels -> (ids, corners)"""
    dist = K[0, 0] * SQUARE / square_px
    ids, corners = [], []
    for g in range(n):
        gx, gy = g % nx, g // nx
        shift = ((gx + 0.5) * W / nx - W / 2, (gy + 0.5) * H / ny - H / 2)
        R, t = diamond_pose((0.0, 0.0, 0.0), dist, roll_deg=0.0, shift_px=shift)
        i, c = hand_diamond([(first_id + 4 * g + q) % 1000 for q in range(4)], R, t)
        ids += i.tolist()
        corners += list(c)
    return np.array(ids, np.int32), np.array(corners, np.float32)


@functools.lru_cache(maxsize=None)
def case_17() -> Case:
    """68 noise-free markers forming 17 diamonds (markers of 21.6 px): more than one pass of 64 marker lanes and of 16 diamonds"""
    ids, corners = _grid(5, 4, 17, 36.0)
    o = np.random.default_rng(17).permutation(len(ids))
    return Case("17 diamonds", ids[o], corners[o], lambda: two_frame().image)


@functools.lru_cache(maxsize=None)
def case_64() -> Case:
    """256 noise-free markers forming 64 diamonds (markers of 10.8 px): both limits"""
    ids, corners = _grid(8, 8, 64, 18.0)
    o = np.random.default_rng(64).permutation(len(ids))
    return Case("64 diamonds", ids[o], corners[o], lambda: two_frame().image)


def hand_cases() -> list:
    return [case_one(r) for r in ROLLS] + [case_two(), case_three_of_four(), case_equal_ids(), case_margin(), case_17(), case_64()]


def ulps(got, want) -> np.ndarray:
    """|got - want| in units of want's float spacing"""
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float32).astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# every hand-made case is made -- and its margins asserted -- at import
ALL = hand_cases()
