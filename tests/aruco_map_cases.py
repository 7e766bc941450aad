"""The maps, hand-made marker sets and rendered scenes the aruco map tests share (tests/test_aruco_map.py on the CPU,
tests/test_gpu_aruco_map*.py on the device): made once per process, never changed."""
from __future__ import annotations

import functools

import numpy as np

from fiducials_amd import synth
from fiducials_amd.detector import map_entries
from fiducials_amd.dictionary import get_predefined_dictionary
from stag_bundle_cases import D_NONZERO, K, exact_minimiser, project, seeded_pose  # noqa: F401  (the same camera and minimiser)

W, H = 640, 480
NOISE_PX = 0.3
DICT = 6
FACING = np.diag([1.0, -1.0, -1.0])  # a marker (x right, y up, z out of its face) that looks straight into the camera

# ---- hand-made geometry for the kernel tests (no frame).  Lengths and positions are dyadic, so that the corners of a board placed by
# a signed permutation are exact in float as well (ora_project_points takes float object points).
LEN, PITCH = 0.125, 0.1875
PERM_X = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])   # board plane -> the map's plane x = const
PERM_Y = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])  # board plane -> the map's plane y = const
OBLIQUE = synth._rodrigues(np.array([0.3, -0.2, 0.1]))


def fid_corners(length: float) -> np.ndarray:
    """getSingleMarkerObjectPoints (aruco_detect.cpp:151-161) with h as the library makes it: (double)(float)(len / 2)."""
    h = float(np.float32(length / 2))
    return np.array([[-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0]])


def grid_board(n: int, cols: int, Rb=np.eye(3), tb=np.zeros(3), first_id: int = 0, length: float = LEN, pitch: float = PITCH):
    """n markers on a cols-wide grid in the plane z = 0 of a board, the board placed in the map by (Rb, tb): MAP_ENTRY_DTYPE."""
    k = np.arange(n)
    xy = np.stack([(k % cols) * pitch - (cols - 1) * pitch / 2, (k // cols) * pitch - 0.09375, np.zeros(n)], axis=1)
    return map_entries(first_id + k, length, np.broadcast_to(Rb, (n, 3, 3)), xy @ Rb.T + tb)


def corner_of_two_walls(n_a: int, n_b: int, first_id: int = 0):
    """Two planes at right angles, both seen from inside the corner: n_a markers on the wall z = 0 (x >= 0.1), n_b on the wall x = 0
    (z >= 0.1), 0.125 m markers at 0.1875 m pitch."""
    Ry = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])  # the marker's z (out of its face) -> the map's +x
    ta = [(0.125 + (k % 3) * PITCH, (k // 3) * PITCH - 0.09375, 0.0) for k in range(n_a)]
    tb = [(0.0, (k // 3) * PITCH - 0.09375, 0.125 + (k % 3) * PITCH) for k in range(n_b)]
    return map_entries(first_id + np.arange(n_a + n_b), LEN, [np.eye(3)] * n_a + [Ry] * n_b, ta + tb)


def look_at(cam_pos, target):
    """The pose (R, t) of the map in a camera at cam_pos that looks at target with the map's y axis up."""
    z = np.asarray(target, float) - np.asarray(cam_pos, float)
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, -1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ np.asarray(cam_pos, float)


def object_points(entries) -> np.ndarray:
    """(4 n, 3): corners 0..3 of every entry in the map frame, in entry order -- what fid_set_map puts on the device."""
    return np.concatenate([fid_corners(e["len"]) @ e["R"].T + e["t"] for e in entries])


def board_pose(rng, Rb, tb, **kw):
    """A seeded pose of the MAP in the camera such that the board placed by (Rb, tb) faces the camera."""
    Rc, tc = seeded_pose(rng, **kw)
    R = Rc @ FACING @ Rb.T
    return R, tc - R @ tb


def _dist(Ra, ta, Rb, tb) -> float:
    return float(max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max()))


# (name, entries): coplanar boards of 2, 5 and 8 markers whose corners are exact in float, and an oblique one of 5
PLANAR_BOARDS = {
    "flat2": (np.eye(3), np.array([0.25, -0.125, 0.5]), 2, 2),
    "side5": (PERM_X, np.array([0.5, 0.25, -0.125]), 5, 3),
    "floor8": (PERM_Y, np.array([-0.25, 0.5, 0.125]), 8, 4),
    "oblique5": (OBLIQUE, np.array([0.05, -0.02, 0.3]), 5, 3),
}


@functools.lru_cache(maxsize=None)
def planar_board(name: str):
    Rb, tb, n, cols = PLANAR_BOARDS[name]
    e = grid_board(n, cols, Rb, tb)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def planar_cases():
    """(board, D, R, t, object points, exact image points, noisy image points); image points rounded to float as a marker holds them."""
    out = []
    rng = np.random.default_rng(4957)
    for name, (Rb, tb, n, cols) in PLANAR_BOARDS.items():
        P = object_points(planar_board(name))
        for Dv in (np.zeros(5), D_NONZERO):
            for _ in range(2):
                R, t = board_pose(rng, Rb, tb, tz_range=(0.9, 1.5))
                img = project(P, R, t, K, Dv)
                noisy = img + rng.uniform(-NOISE_PX, NOISE_PX, size=img.shape)
                out.append((name, Dv, R, t, P, img.astype(np.float32).astype(np.float64), noisy.astype(np.float32).astype(np.float64)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_gap_to_minimum() -> float:
    """The largest distance between oracle.solve_pnp_points and the exact minimiser of the same reprojection error over the noisy
    planar cases (<= 32 points): what CvLevMarq's stop rule (20 iterations / FLT_EPSILON) leaves."""
    import oracle
    worst = 0.0
    for _, Dv, R, t, P, _, noisy in planar_cases():
        r, tv = oracle.solve_pnp_points(K, Dv, P, noisy)
        Rm, tm = exact_minimiser(P, noisy, R, t, K, Dv)
        worst = max(worst, _dist(synth._rodrigues(r), tv, Rm, tm))
    return worst


def split_markers(img_pts: np.ndarray):
    """image points (4 n, 2) -> corners (n, 4, 2) float32"""
    return np.asarray(img_pts, np.float32).reshape(-1, 4, 2)


# ---- rendered scenes (640 x 480, DICT_5X5_250)
SCENE_LEN = 0.08
POSES = ((0.0, 0.62, 1), (0.3, 0.68, 2), (-0.35, 0.72, 3))  # (tilt about an oblique axis, distance, seed)


def _scene_entries(name: str):
    if name == "2x2":
        return grid_board(4, 2, first_id=10, length=SCENE_LEN, pitch=0.13)
    if name == "3x2":
        return grid_board(6, 3, first_id=20, length=SCENE_LEN, pitch=0.13)
    assert name == "corner"
    Ry = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    ta = [(0.08, -0.065, 0.0), (0.08, 0.065, 0.0)]
    tb = [(0.0, -0.065, 0.08), (0.0, 0.065, 0.08)]
    return map_entries(30 + np.arange(4), SCENE_LEN, [np.eye(3)] * 2 + [Ry] * 2, ta + tb)


@functools.lru_cache(maxsize=None)
def scene_map(name: str):
    e = _scene_entries(name)
    e.setflags(write=False)
    return e


def scene_pose(name: str, pose: int):
    a, dist, _ = POSES[pose]
    if name == "corner":
        c = np.array([0.05, 0.0, 0.05])
        d = synth._rodrigues(np.array([0.0, a * 0.5, 0.0])) @ np.array([1.0, 0.15 * (pose - 1), 1.0])
        return look_at(c + dist * d / np.linalg.norm(d), c)
    R = synth._rodrigues(np.array([a, 0.6 * a, 0.0])) @ synth._rodrigues(np.array([0.0, 0.0, 0.2 * pose])) @ FACING
    return R, np.array([0.01, -0.01, dist])


@functools.lru_cache(maxsize=None)
def scene(name: str, pose: int, without: int = -1) -> synth.ArucoBoardFrame:
    """The scene `name` at camera pose `pose`; without = k: marker k of the map is not in the picture (occluded)."""
    e = scene_map(name)
    keep = [k for k in range(len(e)) if k != without]
    R, t = scene_pose(name, pose)
    fr = synth.make_aruco_board_frame(get_predefined_dictionary(DICT), e["id"][keep], [(float(e["len"][k]), e["R"][k], e["t"][k]) for k in keep], K, R, t,
                                      POSES[pose][2], W, H)
    fr.image.setflags(write=False)
    return fr


SCENES = [(n, p) for n in ("2x2", "3x2", "corner") for p in range(len(POSES))]


def map_points_for(entries, ids) -> np.ndarray:
    """Object points for the markers `ids` in list order."""
    by_id = {int(e["id"]): e for e in entries}
    return np.concatenate([fid_corners(by_id[int(i)]["len"]) @ by_id[int(i)]["R"].T + by_id[int(i)]["t"] for i in ids])
