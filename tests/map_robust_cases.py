"""Planted cases for the consensus map pose (tests/test_map_robust_restatement.py on the CPU, tests/test_gpu_map_robust.py on the
device): the dyadic boards of aruco_map_cases seen from seeded poses with +-0.3 px noise, some markers made WRONG -- their four
corners are those of another place: shifted by at least 25 px, turned a quarter turn about the centre (a wrong yaw in the map), or
moved together rigidly with others.  Each case carries its planted inlier set.  Made once per process, never changed.

check_kept() states the conditions under which a case is kept; they are conditions on the INPUTS, established with the NumPy
restatement alone: it recovers the planted set, every err-versus-threshold decision clears its threshold by more than 1 % either
way, and the best two scores (where there are two) differ by more than 1e-6 relative."""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass, field

import numpy as np

import aruco_map_cases as mc
import camera_model_cases as cm
import map_robust_restatement as rr

INLIER_PX = 4.0  # the header's recommendation

Z5 = (0.0,) * 5


@dataclass(frozen=True)
class Case:
    name: str
    model: int
    D: tuple
    entries: np.ndarray = field(repr=False)   # the map
    ids: np.ndarray = field(repr=False)       # the frame's list
    corners: np.ndarray = field(repr=False)   # (n, 4, 2) float32
    planted: tuple | None                     # LIST indices of the planted inliers; None: no consensus is the planted outcome
    min_markers: int = 2
    inlier_px: float = INLIER_PX


def _shift(c, dx, dy):
    return c + np.array([dx, dy])


def _turn(c):
    return np.roll(c, 1, axis=0)  # the same four points, each taken for its neighbour: a quarter turn about the centre


def _project(model, D, P, R, t):
    return cm.project(model, mc.K, D, R, t, P)


def planted_case(name, entries, R, t, seed, wrong=None, model=cm.PLUMB_BOB, D=Z5, moved=None, keep=None, exact=(), **kw) -> Case:
    """entries seen from (R, t); wrong: {map position: ("shift", dx, dy) | ("turn",)}; moved: (positions, R2, t2) -- those markers'
    corners are what they would be from pose (R2, t2); exact: positions without noise; keep: the map positions in the list."""
    rng = np.random.default_rng(seed)
    n = len(entries)
    P = mc.object_points(entries)
    img = _project(model, D, P, R, t).reshape(n, 4, 2)
    if moved is not None:
        pos, R2, t2 = moved
        img2 = _project(model, D, P, R2, t2).reshape(n, 4, 2)
        for k in pos:
            img[k] = img2[k]
    noise = rng.uniform(-mc.NOISE_PX, mc.NOISE_PX, img.shape)
    for k in exact:
        noise[k] = 0.0
    img = img + noise
    wrong = wrong or {}
    for k, how in wrong.items():
        img[k] = _shift(img[k], *how[1:]) if how[0] == "shift" else _turn(img[k])
    keep = list(range(n)) if keep is None else list(keep)
    follow, planted = kw.pop("follow_moved", False), kw.pop("planted", "auto")
    if planted == "auto":
        bad = set(wrong)
        if moved is not None:
            bad |= (set(range(n)) - set(moved[0])) if follow else set(moved[0])
        planted = tuple(i for i, k in enumerate(keep) if k not in bad and i < rr.MAX_USED)
    c = Case(name, model, tuple(D), entries, entries["id"][keep].astype(np.int32), img[keep].astype(np.float32), planted, **kw)
    c.corners.setflags(write=False)
    return c


def _board(name):
    Rb, tb, n, cols = mc.PLANAR_BOARDS[name]
    return mc.planar_board(name), Rb, tb


def _pose(seed, name, **kw):
    _, Rb, tb = _board(name)
    return mc.board_pose(np.random.default_rng(seed), Rb, tb, **kw)


def _grid(n, cols):
    return mc.grid_board(n, cols, np.eye(3), np.array([0.0, 0.0, 0.0]))


def _grid_pose(seed, tz):
    Rc, tc = mc.seeded_pose(np.random.default_rng(seed), tz_range=(tz, tz * 1.05), tilt_deg=(10.0, 25.0))
    return Rc @ mc.FACING, tc


def _wall_pose(seed):
    rng = np.random.default_rng(seed)
    eye = np.array([0.2, 0.0, 0.2]) + rng.uniform(0.7, 1.1) * mc.synth._rodrigues(rng.uniform(-0.25, 0.25, 3)) @ np.array([0.7, 0.1, 0.7])
    return mc.look_at(eye, [0.2, 0.0, 0.2])


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {}

    def add(c):
        assert c.name not in out
        out[c.name] = c

    flat2, floor8, side5, obl5 = (mc.planar_board(b) for b in ("flat2", "floor8", "side5", "oblique5"))
    far = {"tz_range": (0.9, 1.5)}
    # n = 1
    add(planted_case("n1_min1", flat2, *_pose(11, "flat2", **far), 11, keep=[0], min_markers=1))
    add(planted_case("n1_min2", flat2, *_pose(11, "flat2", **far), 11, keep=[0], planted=None))
    # n = 2
    add(planted_case("n2_agree", flat2, *_pose(12, "flat2", **far), 12))
    add(planted_case("n2_disagree", flat2, *_pose(12, "flat2", **far), 12, wrong={1: ("shift", 40.0, -30.0)}, planted=None))
    # n = 3, each position the outlier in turn; side5's first three.  The camera is nearest to ... whichever: the largest is named below
    for bad in range(3):
        add(planted_case(f"n3_bad{bad}", side5[:3], *_pose(13, "side5", **far), 13 + bad, wrong={bad: ("shift", -35.0, 28.0)}))
    # 8 markers, 3 incoherent outliers: coplanar, oblique (5 with 2), and two walls with one wall's marker wrong
    add(planted_case("floor8_3bad", floor8, *_pose(14, "floor8", **far), 14, wrong={1: ("shift", 30.0, 26.0), 4: ("turn",), 6: ("shift", -45.0, 5.0)}))
    add(planted_case("floor8_3bad_D", floor8, *_pose(15, "floor8", **far), 15, D=tuple(mc.D_NONZERO),
                     wrong={0: ("turn",), 3: ("shift", 5.0, -38.0), 7: ("shift", 27.0, 27.0)}))
    add(planted_case("oblique5_2bad", obl5, *_pose(16, "oblique5", **far), 16, wrong={2: ("turn",), 4: ("shift", 31.0, -29.0)}))
    walls = mc.corner_of_two_walls(3, 3)
    add(planted_case("walls33_1bad", walls, *_wall_pose(17), 17, wrong={4: ("shift", 33.0, 30.0)}))
    add(planted_case("walls33_2bad", walls, *_wall_pose(18), 18, wrong={1: ("turn",), 5: ("shift", -28.0, 41.0)}))
    # 8 markers, 5 moved together rigidly: the consensus follows the five
    R8, t8 = _pose(19, "floor8", **far)
    R8b = R8 @ mc.synth._rodrigues(np.array([0.0, 0.12, 0.0]))
    add(planted_case("floor8_5moved", floor8, R8, t8, 19, moved=((0, 2, 3, 5, 7), R8b, t8 + np.array([0.09, -0.05, 0.06])), follow_moved=True))
    # n = 64, 65, 256, 257 (grids at 0.1875 m pitch far from the camera; no distortion, most corners are outside a 640 x 480 frame)
    for n, cols, tz, bad, seed in ((64, 8, 2.5, (3, 40, 63), 84), (256, 16, 4.5, (5, 64, 130, 255), 277), (257, 16, 4.5, (2, 70, 200, 256), 277)):
        g = _grid(n, cols)
        wrong = {k: (("shift", 30.0 + k % 7, -27.0 - k % 5) if i % 2 == 0 else ("turn",)) for i, k in enumerate(bad)}
        add(planted_case(f"grid{n}", g, *_grid_pose(seed, tz), seed, wrong=wrong))
    # 65: the last marker is half the size of the others, so it has the smallest area and is not a hypothesis; its corners carry no
    # noise, so it WOULD win if it were one (test_map_robust_restatement asserts both)
    g65 = _grid(65, 13).copy()
    g65["len"][64] = mc.LEN / 2
    add(planted_case("grid65", g65, *_grid_pose(85, 2.6), 85, wrong={3: ("shift", 29.0, 31.0), 63: ("turn",)}, exact=(64,)))
    # list bookkeeping: unmapped ids and an id seen twice between the used markers; more than 16 outliers
    add(_bookkeeping())
    g40 = _grid(40, 8)
    add(planted_case("grid40_18bad", g40, *_grid_pose(31, 2.2), 31, wrong={k: ("shift", 26.0 + k, -(25.0 + 2 * k)) for k in range(1, 37, 2)}))
    # camera models
    add(planted_case("rational_floor8", floor8, *_pose(32, "floor8", **far), 32, model=cm.RATIONAL, D=cm.SETS["prism12"][1],
                     wrong={2: ("shift", 30.0, 30.0), 5: ("turn",)}))
    add(planted_case("fisheye_floor8", floor8, *_pose(33, "floor8", **far), 33, model=cm.EQUIDISTANT, D=cm.SETS["fe_kb"][1],
                     wrong={1: ("turn",), 6: ("shift", -32.0, 27.0)}))
    # an equidistant frame with one marker past 89 degrees (theta_d = |u - cx| / fx > 1.6): the plain call voids the frame
    add(planted_case("fisheye_past89", floor8, *_pose(34, "floor8", **far), 34, model=cm.EQUIDISTANT, D=(0.0, 0.0, 0.0, 0.0),
                     wrong={3: ("shift", 1500.0, 0.0)}))
    # a re-admission case (searched on the CPU: the seed is the result of the search, see readmission_search)
    add(readmission_case(READMISSION_SEED))
    # the most solves a kept case was found to take: four, stable at the fourth (test_map_robust_restatement says what was searched)
    add(dataclasses.replace(readmission_case(FOUR_SOLVES_SEED), name="four_solves", inlier_px=0.45))
    return out


def _area(c):
    return abs(sum(c[i][0] * c[(i + 1) % 4][1] - c[(i + 1) % 4][0] * c[i][1] for i in range(4)))


def _bookkeeping() -> Case:
    """floor8 (ids 0..7) with one shifted marker; the list also holds ids the map does not name (100, 101) and id 5 twice (both
    left out), placed between the used markers: list indices and used positions differ."""
    base = planted_case("tmp", mc.planar_board("floor8"), *_pose(35, "floor8", tz_range=(0.9, 1.5)), 35, wrong={6: ("shift", 36.0, -25.0)})
    order = [0, ("x", 100), 1, 5, 2, ("x", 101), 3, 5, 4, 6, 7]
    ids, cor = [], []
    for o in order:
        if isinstance(o, tuple):
            ids.append(o[1])
            cor.append(base.corners[0] + 11.0)
        else:
            ids.append(int(base.ids[o]))
            cor.append(base.corners[o])
    planted = tuple(i for i, o in enumerate(order) if not isinstance(o, tuple) and o not in (5, 6))
    c = Case("bookkeeping", base.model, base.D, base.entries, np.array(ids, np.int32), np.array(cor, np.float32), planted)
    c.corners.setflags(write=False)
    return c


# ---- re-admission: a long row seen from far away.  The winner's one-marker pose has a lever arm: markers far from it miss the first
# threshold max(inlier_px, 3 score) although they are right, and come back after the first solve.
FOUR_SOLVES_SEED = 146
READMISSION_SEED = 2  # (readmission_search(1, 120) returned it)


def readmission_case(seed: int) -> Case:
    g = mc.grid_board(12, 12, np.eye(3), np.zeros(3))
    R, t = _grid_pose(seed, 2.4)
    return planted_case("readmission", g, R, t, seed, wrong={4: ("shift", 30.0, 26.0)})


def readmission_search(first: int = 1, last: int = 400):
    """The first seed whose case is kept and has >= 2 solves and a marker outside I_0 inside the result."""
    for seed in range(first, last):
        c = readmission_case(seed)
        try:
            r = check_kept(c)
        except AssertionError:
            continue
        if r["rounds"] >= 2 and set(r["inliers"]) - set(r["I0"]):
            return seed, r
    return None, None


def restate(c: Case, **kw) -> dict:
    return rr.restate(c.model, mc.K, c.D, c.entries, c.ids, c.corners, c.inlier_px, c.min_markers, **kw)


@functools.lru_cache(maxsize=None)
def restated(name: str) -> dict:
    return check_kept(cases()[name])


def check_kept(c: Case) -> dict:
    """Assert the keep conditions of the module docstring on case c; returns the restatement's result."""
    r = restate(c)
    for e, thr in r["decisions"]:
        assert abs(e - thr) > 0.01 * thr, (c.name, "a decision within 1 % of its threshold", e, thr)
    if c.planted is None:
        assert r["status"] == rr.NO_CONSENSUS, (c.name, r["status"])
    else:
        assert r["status"] == rr.OK and tuple(r["used"][k] for k in r["inliers"]) == c.planted, (c.name, r["inliers"], c.planted)
    s = sorted(r["scores"].values())
    assert len(s) < 2 or s[1] - s[0] > 1e-6 * s[1], (c.name, "the best two scores are too close", s[:2])
    return r
