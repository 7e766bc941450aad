"""The pose covariance (include/fid_abi.h, "pose covariance") stated in float64 NumPy, and the cases of test_gpu_pose_cov.py.  No test
functions and no GPU.

reference_cov evaluates sigma^2 (J^T J)^-1 at the pose HANDED IN, with camera_model_cases.complex_step_jacobian for J, and carries it
into the geometry_msgs/PoseWithCovariance convention with a matrix A that is NOT the header's closed form: A and B here are central
differences (five-point stencil) of log(R' R^T) and of the camera's pose in the map, so a wrong closed form on the device -- or a
wrong one in the header -- shows.  test_pose_cov_reference.py holds the closed forms to these.

The tolerance of the device test is not chosen.  Its yardstick is the disagreement of two float64 CPU evaluations of (J^T J)^-1 that
differ only in the order of their operations -- numpy.linalg.inv(J^T J) and a Cholesky inverse of the diagonally scaled matrix --
over the test's own cases, as whitened_dev; TOL is 100 x that figure (the margin: a third operation order on the device, and its
analytic Jacobian against the complex-step one), never above TOL_CAP.  A case whose own figure x 100 exceeds the cap is too
ill-conditioned for the test and is replaced, not excused."""
from __future__ import annotations

import functools

import numpy as np

import camera_model_cases as cm
import pose_cases as pc

TOL_CAP = 1e-6
# TOL is tol(): 100 x cpu_disagreement(), computed from the cases at hand.  As measured: the two CPU inverses disagree by 5.11e-13, so
# TOL = 5.11e-11.
TOL_MEASURED = 5.11e-11
# measured on the device (MI355X): the largest whitened deviation from reference_cov at the device's own poses over every case of
# test_gpu_pose_cov.py -- cov_rt 8.86e-13 (a-posteriori, marker 3), cov_pose 2.10e-12 (the map pose) and cov_cam_pose 2.19e-12 (frame 0
# of the two-frame map batch)
DEVICE_MEASURED = "whitened deviation <= 2.19e-12 (cov_rt <= 8.86e-13, cov_pose <= 2.10e-12, cov_cam_pose <= 2.19e-12)"


# ---------------------------------------------------------------------------------------------- rotations
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_log(R) -> np.ndarray:
    """The rotation vector of a rotation NEAR the identity (angle well below pi): the axis from the antisymmetric part, the angle
    by atan2 of its norm and the trace."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    s = float(np.linalg.norm(w))
    c = (np.trace(R) - 1.0) * 0.5
    if s < 1e-300:
        return w
    return w * (np.arctan2(s, c) / s)


def _stencil(f, x, h):
    """df/dx_j by the five-point central difference, as columns."""
    x = np.asarray(x, dtype=np.float64)
    cols = []
    for j in range(len(x)):
        e = np.zeros(len(x))
        e[j] = h
        cols.append((-f(x + 2 * e) + 8.0 * f(x + e) - 8.0 * f(x - e) + f(x - 2 * e)) / (12.0 * h))
    return np.stack(cols, axis=1)


def A_numeric(rvec, h: float = 1e-3) -> np.ndarray:
    """d(t, theta) / d(rvec, tvec) with R(r + dr) = Exp(dtheta) R(r): central differences of log(R(r + dr) R(r)^T)."""
    R0 = pc.rodrigues(rvec)
    Jl = _stencil(lambda r: so3_log(pc.rodrigues(r) @ R0.T), rvec, h)
    A = np.zeros((6, 6))
    A[:3, 3:] = np.eye(3)
    A[3:, :3] = Jl
    return A


def B_numeric(rvec, tvec, h: float = 1e-3) -> np.ndarray:
    """d(camera pose in the map) / d(pose), both as (translation, rotation about the parent's axes): the pose perturbed as
    (t + dt, Exp(dtheta) R), the camera (R^T, -R^T t) read as (cam_t' - cam_t, log(cam_R' cam_R^T)); central differences."""
    R0 = pc.rodrigues(rvec)
    t0 = np.asarray(tvec, dtype=np.float64)
    cR0, ct0 = R0.T, -R0.T @ t0

    def cam(x):
        R = pc.rodrigues(x[3:]) @ R0 if np.linalg.norm(x[3:]) > 0 else R0
        t = t0 + x[:3]
        return np.concatenate([-R.T @ t - ct0, so3_log(R.T @ cR0.T)])

    return _stencil(cam, np.zeros(6), h)


def A_closed(rvec) -> np.ndarray:
    """fid_abi.h's closed form: A = [[0, I], [J_l(rvec), 0]]."""
    r = np.asarray(rvec, dtype=np.float64)
    th = float(np.linalg.norm(r))
    rx = hat(r)
    if th < 1e-4:
        Jl = np.eye(3) + 0.5 * rx + rx @ rx / 6.0
    else:
        Jl = np.eye(3) + (1.0 - np.cos(th)) / th ** 2 * rx + (th - np.sin(th)) / th ** 3 * (rx @ rx)
    A = np.zeros((6, 6))
    A[:3, 3:] = np.eye(3)
    A[3:, :3] = Jl
    return A


def B_closed(rvec, tvec) -> np.ndarray:
    """fid_abi.h's closed form: B = [[-R^T, -R^T [t]x], [0, -R^T]]."""
    R = pc.rodrigues(rvec)
    B = np.zeros((6, 6))
    B[:3, :3] = -R.T
    B[:3, 3:] = -R.T @ hat(np.asarray(tvec, dtype=np.float64))
    B[3:, 3:] = -R.T
    return B


# ---------------------------------------------------------------------------------------------- the reference
def normal_matrix(model, K, D, rvec, tvec, obj, img):
    """J^T J and |e|^2 at (rvec, tvec): J by the complex step, e = projection - img, both unrounded."""
    obj = np.asarray(obj, dtype=np.float64).reshape(-1, 3)
    J = cm.complex_step_jacobian(model, K, D, rvec, tvec, obj).reshape(-1, 6)
    e = (cm.project(model, K, D, np.asarray(rvec, dtype=np.float64), tvec, obj) - np.asarray(img, dtype=np.float64).reshape(-1, 2)).reshape(-1)
    return J.T @ J, float(e @ e)


def reference_cov(model, K, D, rvec, tvec, obj, img, sigma_px):
    """-> cov_rt, cov_pose, sigma2 at the pose handed in (fid_abi.h's definitions; A by central differences)."""
    JtJ, e2 = normal_matrix(model, K, D, rvec, tvec, obj, img)
    n = len(np.asarray(obj).reshape(-1, 3))
    sigma2 = float(sigma_px) ** 2 if sigma_px > 0 else e2 / (2 * n - 6)
    cov_rt = sigma2 * np.linalg.inv(JtJ)
    cov_rt = 0.5 * (cov_rt + cov_rt.T)
    A = A_numeric(rvec)
    return cov_rt, A @ cov_rt @ A.T, sigma2


def reference_cov_cam(rvec, tvec, cov_pose):
    """cov_cam_pose from cov_pose, B by central differences."""
    B = B_numeric(rvec, tvec)
    return B @ cov_pose @ B.T


def whitened_dev(S, S_ref) -> float:
    """max |L^-1 S L^-T - I| with S_ref = L L^T: the deviation in units of the reference's own standard deviations."""
    L = np.linalg.cholesky(np.asarray(S_ref, dtype=np.float64))
    Li = np.linalg.inv(L)
    return float(np.abs(Li @ np.asarray(S, dtype=np.float64) @ Li.T - np.eye(len(L))).max())


def inverse_by_scaled_cholesky(M):
    """M^-1 in another operation order: M = D C D with unit-diagonal C, C = L L^T, M^-1 = D^-1 L^-T L^-1 D^-1."""
    d = np.sqrt(np.diag(M))
    L = np.linalg.cholesky(M / np.outer(d, d))
    Li = np.linalg.inv(L)
    return (Li.T @ Li) / np.outer(d, d)


# ---------------------------------------------------------------------------------------------- the cases
# the four camera x coefficient sets every k_pose case runs under: name -> (model, D)
CAMERA_SETS = {"barrel": (cm.PLUMB_BOB, pc.DISTORTIONS["barrel"]), "kinect": cm.SETS["kinect"], "prism12": cm.SETS["prism12"], "fe_kb": cm.SETS["fe_kb"]}
CAM = "hd"
NODE_LEN = 0.14
OVERRIDE_LEN = 0.05
# (id, length, side px, tilt degrees): one with a length override, one small and far, one large and oblique; the fourth is the
# marker of the second frame
MARKERS = ((7, OVERRIDE_LEN, 80.0, 45.0), (1, NODE_LEN, 25.0, 20.0), (2, NODE_LEN, 300.0, 65.0), (3, NODE_LEN, 80.0, 45.0))
CENTRES = ((620.0, 400.0), (1300.0, 330.0), (900.0, 700.0), (1000.0, 500.0))  # pixels: inside the middle of the hd frame
NOISE_PX = 0.05


def _marker_pose(model, D, length, side, tilt, centre, seed):
    fx, fy, cx, cy, _, _ = pc.CAMERAS[CAM]
    rng = np.random.default_rng([20261018, seed])
    axis_dir, roll = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-np.pi, np.pi)
    z = 0.5 * (fx + fy) * length / side
    nx, ny = cm.undistort_exact(model, D, (centre[0] - cx) / fx, (centre[1] - cy) / fy)
    R = pc.rodrigues(np.array([np.cos(axis_dir), np.sin(axis_dir), 0.0]) * np.deg2rad(tilt)) @ pc.rodrigues([0.0, 0.0, roll]) @ np.diag([1.0, -1.0, -1.0])
    return R, np.array([nx * z, ny * z, z]), rng.standard_normal((4, 2))


@functools.lru_cache(maxsize=None)
def marker_cases(set_name: str, noisy: bool = False):
    """The four markers under one camera set: (ids, lengths, corners (4, 4, 2) float32, object points, R, t) -- corners projected by
    the NumPy model, with NOISE_PX of noise when noisy, rounded to float32 as a fid_marker holds them."""
    model, D = CAMERA_SETS[set_name]
    K = pc.camera_matrix(CAM)
    ids, lens, corners, objs, Rs, ts = [], [], [], [], [], []
    for k, ((mid, length, side, tilt), centre) in enumerate(zip(MARKERS, CENTRES)):
        R, t, noise = _marker_pose(model, D, length, side, tilt, centre, k)
        obj = pc.square_object_points(length)
        c = cm.project(model, K, D, R, t, obj) + (NOISE_PX * noise if noisy else 0.0)
        ids.append(mid)
        lens.append(length)
        corners.append(c.astype(np.float32))
        objs.append(obj)
        Rs.append(R)
        ts.append(t)
    return np.array(ids, np.int32), lens, np.stack(corners), objs, Rs, ts


def rvec_of(R) -> np.ndarray:
    """Rotation matrix -> vector (angle inside (0, pi))."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    s = float(np.linalg.norm(w))
    return w * (np.arctan2(s, (np.trace(R) - 1.0) * 0.5) / s)


# ---- k_stag_pose: the 5-point record of two markers (vga x mild, marker size 0.18): a frontal one and an oblique one
STAG_K, STAG_D, STAG_SIZE = pc.camera_matrix("vga"), pc.dist_coeffs("mild"), 0.18


@functools.lru_cache(maxsize=None)
def stag_cases(noisy: bool = False):
    """Stand-ins, for the yardstick, of the rendered frame's markers that the device test poses (fid_stag_pose_last* takes the markers
    of a detect call): the same camera, size and five points at a frontal and an oblique pose.
    -> (image points (2, 5, 2): centre then corners, object points (5, 3), Rs, ts)."""
    fx, fy, cx, cy, _, _ = pc.CAMERAS["vga"]
    obj = pc.stag_object_points(STAG_SIZE)
    rng = np.random.default_rng(20261019)
    pts, Rs, ts = [], [], []
    for side, tilt, centre in ((90.0, 15.0, (200.0, 180.0)), (140.0, 50.0, (430.0, 300.0))):
        z = 0.5 * (fx + fy) * STAG_SIZE / side
        R = pc.rodrigues(np.array([np.cos(0.7), np.sin(0.7), 0.0]) * np.deg2rad(tilt)) @ pc.rodrigues([0.0, 0.0, 0.4]) @ np.diag([1.0, -1.0, -1.0])
        t = np.array([(centre[0] - cx) / fx * z, (centre[1] - cy) / fy * z, z])
        pts.append(cm.project(cm.PLUMB_BOB, STAG_K, STAG_D, R, t, obj) + (NOISE_PX * rng.standard_normal((5, 2)) if noisy else 0.0))
        Rs.append(R)
        ts.append(t)
    return np.stack(pts), obj, Rs, ts


# ---- k_stag_bundle_pose: a coplanar 2-tag bundle (ids 0, 1), a 2-tag bundle on two faces (ids 2, 3), a bundle whose tag (id 4) is
# not among the markers; stag_bundle_cases' geometry and camera
@functools.lru_cache(maxsize=None)
def bundle_cases(noisy: bool = False):
    """-> (tag corners per bundle [(2, 4, 3), (2, 4, 3), (1, 4, 3)], per posed bundle: object points (10, 3), image points (10, 2), R, t)."""
    import stag_bundle_cases as bc

    boards = [bc.oblique_board(2), bc.two_faces(2), bc.oblique_board(3)[2:3]]
    rng = np.random.default_rng(20261020)
    posed = []
    for b in range(2):
        P = bc.tags_points(boards[b])
        R, t = bc.seeded_pose(rng)
        if b == 1:  # both faces towards the camera
            R = R @ pc.rodrigues([0.0, -np.pi / 4, 0.0]) @ np.diag([1.0, -1.0, -1.0]) @ pc.rodrigues([0.0, 0.0, 0.0])
        img = bc.project(P, R, t, bc.K, bc.D_NONZERO) + (NOISE_PX * rng.standard_normal((len(P), 2)) if noisy else 0.0)
        posed.append((P, img, R, t))
    return boards, posed


# ---- k_map_pose: a 4-marker board of which 3 are seen in the first frame; the second frame holds one marker the map does not name
@functools.lru_cache(maxsize=None)
def map_case(noisy: bool = False):
    """-> (map entries (4), seen ids, object points (12, 3) of the three seen, image points (12, 2), R, t)."""
    import aruco_map_cases as mc

    e = mc.grid_board(4, 2, mc.OBLIQUE, np.array([0.0625, -0.03125, 0.25]))
    rng = np.random.default_rng(20261021)
    R, t = mc.board_pose(rng, mc.OBLIQUE, np.array([0.0625, -0.03125, 0.25]))
    seen = [0, 1, 3]
    P = mc.object_points(e[seen])
    img = mc.project(P, R, t, mc.K, mc.D_NONZERO) + (NOISE_PX * rng.standard_normal((len(P), 2)) if noisy else 0.0)
    return e, np.array(seen, np.int32), P, img.astype(np.float32).astype(np.float64), R, t


def all_normal_matrices():
    """J^T J of every case of the device test at its generating pose."""
    out = []
    for set_name, (model, D) in CAMERA_SETS.items():
        K = pc.camera_matrix(CAM)
        _, _, corners, objs, Rs, ts = marker_cases(set_name)
        for c, obj, R, t in zip(corners, objs, Rs, ts):
            out.append(normal_matrix(model, K, D, rvec_of(R), t, obj, c)[0])
    pts, obj, Rs, ts = stag_cases()
    for p, R, t in zip(pts, Rs, ts):
        out.append(normal_matrix(cm.PLUMB_BOB, STAG_K, STAG_D, rvec_of(R), t, obj, p)[0])
    import stag_bundle_cases as bc

    for P, img, R, t in bundle_cases()[1]:
        out.append(normal_matrix(cm.PLUMB_BOB, bc.K, bc.D_NONZERO, rvec_of(R), t, P, img)[0])
    _, _, P, img, R, t = map_case()
    out.append(normal_matrix(cm.PLUMB_BOB, bc.K, bc.D_NONZERO, rvec_of(R), t, P, img)[0])
    return out


@functools.lru_cache(maxsize=None)
def cpu_disagreement() -> float:
    """The yardstick (module docstring) over every case of the device test at its generating pose: the largest whitened_dev between
    the two CPU inverses of J^T J."""
    worst = 0.0
    for JtJ in all_normal_matrices():
        a, b = np.linalg.inv(JtJ), inverse_by_scaled_cholesky(JtJ)
        worst = max(worst, whitened_dev(a, 0.5 * (b + b.T)))
    return worst


def tol() -> float:
    """100 x the CPU figure of the cases at hand, which must stay under the cap."""
    fig = cpu_disagreement()
    t = 100.0 * fig
    print(f"\npose covariance: two float64 CPU inverses of J^T J disagree by {fig:.3g} (whitened) over the cases; TOL = {t:.3g} (cap {TOL_CAP:g})")
    assert t <= TOL_CAP, "a case is too ill-conditioned for this test: replace it"
    return t
