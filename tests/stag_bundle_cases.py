"""The scenes and layouts the bundle tests share (tests/test_stag_bundles.py on the CPU, tests/test_gpu_stag_bundles*.py on the
device): rendered once per process, never changed."""
from __future__ import annotations

import functools

import numpy as np

from fiducials_amd import stag as fstag
from fiducials_amd import synth

W, H = 640, 480
K = np.array([[466.7, 0, 320.0], [0, 466.7, 240.0], [0, 0, 1.0]])
D_NONZERO = np.array([0.05, -0.02, 0.001, -0.0005, 0.0])
TAG_PX, TAG_SIZE, GAP_PX = 96, 0.08, 40
# (library, ids, cols, rows)
BOARDS = {"hd21_2x2": (21, (0, 1, 2, 3), 2, 2), "hd21_3x2": (21, (0, 1, 2, 3, 4, 5), 3, 2), "hd11_2x2": (11, (0, 1, 2, 3), 2, 2)}
POSES = ((0.0, 0.45, 1), (0.35, 0.50, 2), (0.5, 0.55, 3))  # (a, t_z, seed)


def pose_of(a: float, tz: float):
    R = synth._rodrigues(np.array([a, 0.6 * a, 0.0])) @ synth._rodrigues(np.array([0.0, 0.0, 0.4]))
    return R, np.array([0.01, -0.01, tz])


@functools.lru_cache(maxsize=None)
def scene(board: str, pose: int) -> synth.StagBoardFrame:
    hd, ids, cols, rows = BOARDS[board]
    a, tz, seed = POSES[pose]
    R, t = pose_of(a, tz)
    fr = synth.make_stag_board_frame(hd, ids, cols, rows, K, R, t, seed, W, H, TAG_PX, TAG_SIZE, GAP_PX)
    fr.image.setflags(write=False)
    return fr


def all_scenes():
    return [(b, p) for b in BOARDS for p in range(len(POSES))]


def hd21_scenes():
    return [(b, p) for b in ("hd21_2x2", "hd21_3x2") for p in range(len(POSES))]


def board_points(fr: synth.StagBoardFrame, ids_in_order) -> np.ndarray:
    """Object points of solvePnpBundle for the tags `ids_in_order`: per tag centre, c0..c3 -- centre and c3 as the loader makes them
    from c0..c2 (load_yaml_tags.h:28-30)."""
    out = []
    for i in ids_in_order:
        c = fr.corners_board[list(fr.ids).index(int(i))]
        out.append((c[2] + c[0]) / 2)
        out.extend([c[0], c[1], c[2], c[0] + (c[2] - c[1])])
    return np.array(out)


def marker_points(markers: np.ndarray) -> np.ndarray:
    """Image points of solvePnpBundle for markers (MARKER_DTYPE) in list order: Marker::center, Marker::corners."""
    return np.concatenate([np.concatenate([m["center"][None, :], m["corners"]], axis=0) for m in markers], axis=0)


def ref_markers_as_dtype(ref: np.ndarray) -> np.ndarray:
    """oracle.stag_ref.detect_markers rows as MARKER_DTYPE (id, corners, center)."""
    m = np.zeros(len(ref), fstag.MARKER_DTYPE)
    m["id"] = ref[:, 0].astype(np.int32)
    m["corners"] = ref[:, 1:9].reshape(-1, 4, 2)
    m["center"] = ref[:, 9:11]
    return m


def angle_deg(n1, n2) -> float:
    c = float(np.dot(n1, n2) / (np.linalg.norm(n1) * np.linalg.norm(n2)))
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, c)))))


# ---- hand-made geometry for the kernel tests (no frame)
def oblique_board(n_tags: int):
    """A 3 x 2 board of 0.08 m tags at 0.10 m pitch, placed obliquely in the bundle frame (rotated by Rod((0.3, -0.2, 0.1)), shifted by
    (0.05, -0.02, 0.3)): corners (n_tags, 4, 3) of its first n_tags tags, c0..c3 clockwise."""
    Rb = synth._rodrigues(np.array([0.3, -0.2, 0.1]))
    tb = np.array([0.05, -0.02, 0.3])
    out = []
    for k in range(n_tags):
        x0, y0 = (k % 3) * 0.10 - 0.14, (k // 3) * 0.10 - 0.09
        c = np.array([[x0, y0, 0], [x0 + 0.08, y0, 0], [x0 + 0.08, y0 + 0.08, 0], [x0, y0 + 0.08, 0]], float)
        out.append(c @ Rb.T + tb)
    return np.array(out)


def two_faces(n_tags: int):
    """Tags on two faces at 90 degrees (a tool with tags on two sides): n_tags / 2 on the plane z = 0, n_tags / 2 on the plane x = 0,
    0.08 m tags at 0.10 m pitch; corners (n_tags, 4, 3)."""
    half = n_tags // 2
    out = []
    for k in range(half):
        x0, y0 = 0.02 + (k % 3) * 0.10, (k // 3) * 0.10 - 0.09
        out.append(np.array([[x0, y0, 0], [x0 + 0.08, y0, 0], [x0 + 0.08, y0 + 0.08, 0], [x0, y0 + 0.08, 0]], float))
    for k in range(n_tags - half):
        z0, y0 = 0.02 + (k % 3) * 0.10, (k // 3) * 0.10 - 0.09
        out.append(np.array([[0, y0, z0 + 0.08], [0, y0, z0], [0, y0 + 0.08, z0], [0, y0 + 0.08, z0 + 0.08]], float))
    return np.array(out)


def tags_points(corners: np.ndarray) -> np.ndarray:
    """centre, c0..c3 per tag, made from c0..c2 as the loader makes them."""
    out = []
    for c in corners:
        out.append((c[2] + c[0]) / 2)
        out.extend([c[0], c[1], c[2], c[0] + (c[2] - c[1])])
    return np.array(out)


def seeded_pose(rng, tz_range=(0.6, 1.2), tilt_deg=(15.0, 35.0)):
    tilt = np.deg2rad(rng.uniform(*tilt_deg))
    tdir = rng.uniform(0, 2 * np.pi)
    theta = rng.uniform(-np.pi, np.pi)
    R = synth._rodrigues(np.array([np.cos(tdir), np.sin(tdir), 0.0]) * tilt) @ synth._rodrigues(np.array([0, 0, theta]))
    t = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(*tz_range)])
    return R, t


def project(P, R, t, Kc, Dv):
    """cv::projectPoints with the plumb-bob model (k1, k2, p1, p2, k3)."""
    Pc = P @ R.T + t
    x, y = Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2]
    k1, k2, p1, p2, k3 = Dv
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([Kc[0, 0] * xd + Kc[0, 2], Kc[1, 1] * yd + Kc[1, 2]], axis=1)


def markers_from_points(ids, img5: np.ndarray) -> np.ndarray:
    """MARKER_DTYPE records from per-tag image points (n, 5, 2): centre, c0..c3."""
    m = np.zeros(len(ids), fstag.MARKER_DTYPE)
    m["id"] = np.asarray(ids, np.int32)
    m["center"] = img5[:, 0]
    m["corners"] = img5[:, 1:]
    return m


def _residual_and_jacobian(P, img, R, t, Kc, Dv):
    """Reprojection residuals (2n,) and their exact Jacobian (2n, 6) with respect to (w, dt) in exp(w) R, t + dt."""
    Q = P @ R.T
    Pc = Q + t
    Z = Pc[:, 2]
    x, y = Pc[:, 0] / Z, Pc[:, 1] / Z
    k1, k2, p1, p2, k3 = Dv
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3
    dcd = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    res = np.stack([Kc[0, 0] * xd + Kc[0, 2], Kc[1, 1] * yd + Kc[1, 2]], axis=1) - img
    dxd = np.stack([cd + 2 * x * x * dcd + 2 * p1 * y + 6 * p2 * x, 2 * x * y * dcd + 2 * p1 * x + 2 * p2 * y], axis=1)
    dyd = np.stack([2 * x * y * dcd + 2 * p1 * x + 2 * p2 * y, cd + 2 * y * y * dcd + 6 * p1 * y + 2 * p2 * x], axis=1)
    n = len(P)
    dxy = np.zeros((n, 2, 3))  # d(x, y) / dPc
    dxy[:, 0, 0] = 1 / Z
    dxy[:, 0, 2] = -x / Z
    dxy[:, 1, 1] = 1 / Z
    dxy[:, 1, 2] = -y / Z
    dPc = np.zeros((n, 3, 6))  # dPc / d(w, dt): -[Q]x, I
    dPc[:, 0, 1], dPc[:, 0, 2] = Q[:, 2], -Q[:, 1]
    dPc[:, 1, 0], dPc[:, 1, 2] = -Q[:, 2], Q[:, 0]
    dPc[:, 2, 0], dPc[:, 2, 1] = Q[:, 1], -Q[:, 0]
    dPc[:, 0, 3] = dPc[:, 1, 4] = dPc[:, 2, 5] = 1.0
    dd = np.stack([dxd * Kc[0, 0], dyd * Kc[1, 1]], axis=1)  # (n, 2, 2): d(u, v) / d(x, y)
    J = dd @ dxy @ dPc
    return res.reshape(-1), J.reshape(-1, 6)


def _exp_so3(w):
    """exp([w]x), exact for steps of any size (down to the last bit of a converging iteration)."""
    th = float(np.linalg.norm(w))
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    a = np.sinc(th / np.pi)                    # sin(th) / th
    b = 0.5 * np.sinc(th / (2 * np.pi)) ** 2   # (1 - cos(th)) / th^2
    return np.eye(3) + a * Wx + b * (Wx @ Wx)


def exact_minimiser(P, img, R0, t0, Kc, Dv):
    """The minimum of the reprojection error next to (R0, t0): Gauss-Newton on (rotation increment, t) with the exact Jacobian, run
    until the step is below 1e-14.  Returns (R, t)."""
    R, t = R0.copy(), t0.copy()
    for _ in range(500):
        r0, J = _residual_and_jacobian(P, img, R, t, Kc, Dv)
        step = np.linalg.lstsq(J, -r0, rcond=None)[0]
        R = _exp_so3(step[:3]) @ R
        t = t + step[3:]
        if np.linalg.norm(step) < 1e-14:
            break
    else:
        raise AssertionError("the Gauss-Newton reference did not converge")
    return R, t
