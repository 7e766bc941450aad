"""The rig pose (fid_abi.h: "one rig pose per time step from all cameras of a multi-camera rig") restated in float64 NumPy from the
header's text: the gather over the cameras, the start camera and its single-camera solve, the composition with the extrinsic,
CvLevMarq on the residuals of all cameras with an analytic Jacobian, the record and the covariance.  No test functions, no GPU.

What is NOT the device's arithmetic, and does not have to be: the order of the sums (NumPy's), the eigen-decompositions of the
start (numpy.linalg.eigh for the scatter matrix and the DLT instead of cyclic Jacobi), cv::Rodrigues of a matrix (an SVD).  They
move the START by rounding; CvLevMarq then runs the same ladder from it, and what its stop rule (20 accepted steps, relative step
below FLT_EPSILON) leaves is far below the 1e-6 the device is held to (test_gpu_rig_pose.py measures it against the exact minimum)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import camera_model_cases as cm
from map_robust_restatement import fid_corners, one_marker_pose, undistort

MAX_CAMERAS, MAX_USED = 16, 128
FLT_EPSILON, DBL_EPSILON = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


@dataclass(frozen=True)
class Cam:
    """A camera of a rig: the model with K (3, 3) and D, and the RIG frame in the CAMERA frame, X_cam = R X_rig + t."""
    model: int
    K: np.ndarray
    D: tuple
    R: np.ndarray
    t: np.ndarray

    def alone(self) -> "Cam":
        return Cam(self.model, self.K, self.D, np.eye(3), np.zeros(3))


def from_tf(xyz, quat_xyzw):
    """(R, t) of a Cam from the camera's pose in the rig frame: position and quaternion (x, y, z, w), normalised here."""
    x, y, z, w = np.asarray(quat_xyzw, float) / np.linalg.norm(quat_xyzw)
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return Rq.T, -Rq.T @ np.asarray(xyz, float)


# ---------------------------------------------------------------------------------------------- rotations
def rodrigues(r, jac: bool = False):
    """cvRodrigues2 vector -> matrix; with jac also dR/dr as (3, 3, 3): [i] = dR / dr_i."""
    r = np.asarray(r, float)
    th = float(np.sqrt(r @ r))
    if th < DBL_EPSILON:
        R = np.eye(3)
        if not jac:
            return R
        J = np.zeros((3, 3, 3))
        J[0, 1, 2], J[0, 2, 1] = -1, 1
        J[1, 0, 2], J[1, 2, 0] = 1, -1
        J[2, 0, 1], J[2, 1, 0] = -1, 1
        return R, J
    c, s = np.cos(th), np.sin(th)
    c1, ith = 1 - c, 1 / th
    k = r * ith
    rrt = np.outer(k, k)
    rx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = c * np.eye(3) + c1 * rrt + s * rx
    if not jac:
        return R
    J = np.zeros((3, 3, 3))
    for i in range(3):
        e = np.zeros(3)
        e[i] = 1
        drrt = np.outer(e, k) + np.outer(k, e)
        drx = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
        a0, a1, a2, a3, a4 = -s * k[i], (s - 2 * c1 * ith) * k[i], c1 * ith, (c - s * ith) * k[i], s * ith
        J[i] = a0 * np.eye(3) + a1 * rrt + a2 * drrt + a3 * rx + a4 * drx
    return R, J


def rotvec(R) -> np.ndarray:
    """cv::Rodrigues matrix -> vector: the nearest rotation (U V^T of the SVD), the axis from its antisymmetric part."""
    U, _, Vt = np.linalg.svd(np.asarray(R, float))
    R = U @ Vt
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.sqrt((w @ w) * 0.25))
    c = float(np.clip((np.trace(R) - 1) * 0.5, -1, 1))
    th = np.arccos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        v = np.sqrt(np.maximum((np.diag(R) + 1) * 0.5, 0))
        v[1] *= -1 if R[0, 1] < 0 else 1
        v[2] *= -1 if R[0, 2] < 0 else 1
        if abs(v[0]) < abs(v[1]) and abs(v[0]) < abs(v[2]) and (R[1, 2] > 0) != (v[1] * v[2] > 0):
            v[2] = -v[2]
        return v * (th / np.linalg.norm(v))
    return w * (th / (2 * s))


# ---------------------------------------------------------------------------------------------- the projection through a rig
def _pixel_and_gradient(cam: Cam, Xc: np.ndarray):
    """Camera-frame points (n, 3) -> pixels (n, 2) and d(u, v) / d Xc (n, 2, 3), analytic, under the camera's own model."""
    k = list(cam.D) + [0.0] * (12 - len(cam.D))
    fx, fy, cx, cy = cam.K[0, 0], cam.K[1, 1], cam.K[0, 2], cam.K[1, 2]
    iz = 1 / Xc[:, 2]
    x, y = Xc[:, 0] * iz, Xc[:, 1] * iz
    r2 = x * x + y * y
    if cam.model == cm.EQUIDISTANT:
        r = np.sqrt(r2)
        th = np.arctan(r)
        th2 = th * th
        thd = th * (1 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3]))))
        dthd = 1 + th2 * (3 * k[0] + th2 * (5 * k[1] + th2 * (7 * k[2] + th2 * 9 * k[3])))
        tiny = ~(r > 1e-8)
        rs, r2s = np.where(tiny, 1.0, r), np.where(tiny, 1.0, r2)
        scale = np.where(tiny, 1.0, thd / rs)
        g = np.where(tiny, 0.0, (dthd / (1 + r2) - scale) / r2s)  # d scale = g (x dx + y dy)
        xd, yd = x * scale, y * scale
        xx, xy, yx, yy = scale + x * g * x, x * g * y, y * g * x, scale + y * g * y
    else:
        r4 = r2 * r2
        cd, dcd = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4])), k[0] + 2 * k[1] * r2 + 3 * k[4] * r4
        icd, dicd = np.ones_like(r2), np.zeros_like(r2)
        px = py = dpx = dpy = np.zeros_like(r2)
        if cam.model == cm.RATIONAL:
            den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]))
            icd, dicd = 1 / den, -(k[5] + 2 * k[6] * r2 + 3 * k[7] * r4) / (den * den)
            px, py, dpx, dpy = r2 * (k[8] + r2 * k[9]), r2 * (k[10] + r2 * k[11]), k[8] + 2 * k[9] * r2, k[10] + 2 * k[11] * r2
        f, df = cd * icd, dcd * icd + cd * dicd  # (df, dpx, dpy: with respect to r2)
        xd = x * f + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + px
        yd = y * f + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + py
        xx = f + x * df * 2 * x + 2 * k[2] * y + 6 * k[3] * x + dpx * 2 * x
        xy = x * df * 2 * y + 2 * k[2] * x + 2 * k[3] * y + dpx * 2 * y
        yx = y * df * 2 * x + 2 * k[2] * x + 2 * k[3] * y + dpy * 2 * x
        yy = f + y * df * 2 * y + 6 * k[2] * y + 2 * k[3] * x + dpy * 2 * y
    uv = np.stack([fx * xd + cx, fy * yd + cy], axis=1)
    G = np.zeros((len(Xc), 2, 3))
    G[:, 0, 0], G[:, 0, 1], G[:, 0, 2] = fx * xx * iz, fx * xy * iz, -fx * (xx * x + xy * y) * iz
    G[:, 1, 0], G[:, 1, 1], G[:, 1, 2] = fy * yx * iz, fy * yy * iz, -fy * (yx * x + yy * y) * iz
    return uv, G


def project(cams, pcam, param, P, jac: bool = False):
    """Point p (of camera pcam[p]) projects as proj_c(R_c (R(rvec) M_p + tvec) + t_c): pixels (n, 2); with jac also
    d(u, v) / d(rvec, tvec) as (n, 2, 6), analytic."""
    param = np.asarray(param, float)
    P = np.asarray(P, float).reshape(-1, 3)
    pcam = np.asarray(pcam, int)
    R, dR = rodrigues(param[:3], True)
    Xr = P @ R.T + param[3:]
    uv, J = np.zeros((len(P), 2)), np.zeros((len(P), 2, 6))
    for c in np.unique(pcam):
        sel = np.nonzero(pcam == c)[0]
        cam = cams[c]
        u, G = _pixel_and_gradient(cam, Xr[sel] @ cam.R.T + cam.t)
        uv[sel] = u
        if jac:
            H = G @ cam.R  # d(u, v) / d X_rig
            J[sel, :, 3:] = H
            for i in range(3):
                J[sel, :, i] = np.einsum("nka,na->nk", H, P[sel] @ dR[i].T)
    return (uv, J) if jac else uv


# ---------------------------------------------------------------------------------------------- CvLevMarq
def lev_marq(cams, pcam, P, img, param0):
    """CvLevMarq as fid_pnp.h's LevMarq states it: lambda = 10^lambdaLg10 from -3 inside [-16, 16], ten times the damping while the
    error grows, the stop after 20 accepted steps or on a relative step below FLT_EPSILON.  -> param, and the squared error norms of
    every evaluation, the first being the start's."""
    img = np.asarray(img, float).reshape(-1, 2)

    def evaluate(p, want_j):
        if want_j:
            uv, J = project(cams, pcam, p, P, True)
            e = (uv - img).reshape(-1)
            J = J.reshape(-1, 6)
            return float(e @ e), J.T @ J, J.T @ e
        e = (project(cams, pcam, p, P) - img).reshape(-1)
        return float(e @ e), None, None

    param = np.array(param0, float)
    lg, iters = -3, 0
    e2, S, g = evaluate(param, True)
    costs = [e2]
    while True:
        prev, prev_norm = param.copy(), np.sqrt(e2)
        while True:
            lam = float(np.exp(max(min(lg, 16), -16) * np.log(10.0)))
            param = prev - np.linalg.solve(S + lam * np.diag(np.diag(S)), g)
            e2 = evaluate(param, False)[0]
            costs.append(e2)
            if not (np.sqrt(e2) > prev_norm and lg + 1 <= 16):
                if np.sqrt(e2) > prev_norm:
                    lg += 1
                break
            lg += 1
        lg = max(lg - 1, -16)
        iters += 1
        rel = np.linalg.norm(param - prev) / (np.linalg.norm(prev) + DBL_EPSILON)
        if iters >= 20 or rel < FLT_EPSILON:
            return param, costs
        e2, S, g = evaluate(param, True)


# ---------------------------------------------------------------------------------------------- the start: one camera alone
def _dlt_homography(Mxy, mn):
    """HomographyEstimatorCallback::runKernel on float inputs: centroids, mean-absolute-deviation scales, the eigenvector of the
    smallest eigenvalue of L^T L, de-normalised and scaled to H[2, 2] = 1."""
    n = len(Mxy)
    cm_, cM = mn.mean(0), Mxy.mean(0)
    sm, sM = n / np.abs(mn - cm_).sum(0), n / np.abs(Mxy - cM).sum(0)
    x, y = ((mn - cm_) * sm).T
    X, Y = ((Mxy - cM) * sM).T
    o, z = np.ones(n), np.zeros(n)
    L = np.concatenate([np.stack([X, Y, o, z, z, z, -x * X, -x * Y, -x], 1), np.stack([z, z, z, X, Y, o, -y * X, -y * Y, -y], 1)])
    H0 = np.linalg.eigh(L.T @ L)[1][:, 0].reshape(3, 3)
    H = np.array([[1 / sm[0], 0, cm_[0]], [0, 1 / sm[1], cm_[1]], [0, 0, 1]]) @ H0 @ np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1]])
    return H / H[2, 2]


def solve_one_camera(cam: Cam, P, img, areas):
    """fid_map_pose_cam's solve on one camera's points: (rvec, tvec) of the map in that camera.  Coplanar points
    (cvFindExtrinsicCameraParams2's test): the DLT homography over all of them; else the closed-form pose of the marker with the
    largest image area, the first of equals; then CvLevMarq."""
    P, img = np.asarray(P, float).reshape(-1, 3), np.asarray(img, float).reshape(-1, 2)
    Mc = P.mean(0)
    w, V = np.linalg.eigh((P - Mc).T @ (P - Mc))
    w, Vt = w[::-1], V[:, ::-1].T
    if w[2] / w[1] < 1e-3:
        Rt = Vt.copy()
        if Rt[0, 2] ** 2 + Rt[1, 2] ** 2 < 1e-10:
            Rt = np.eye(3)
        if np.linalg.det(Rt) < 0:
            Rt = -Rt
        tt = -Rt @ Mc
        Mxy = (P @ Rt.T + tt)[:, :2].astype(np.float32).astype(np.float64)
        mn = np.array([undistort(cam.model, cam.K, cam.D, u, v)[:2] for u, v in img]).astype(np.float32).astype(np.float64)
        H = _dlt_homography(Mxy, mn)
        n1, n2 = np.linalg.norm(H[:, 0]), np.linalg.norm(H[:, 1])
        t3 = H[:, 2] * 2 / (n1 + n2)
        r1, r2 = H[:, 0] / n1, H[:, 1] / n2
        Rh = rodrigues(rotvec(np.stack([r1, r2, np.cross(r1, r2)], axis=1)))
        R0, t0 = Rh @ Rt, Rh @ tt + t3
    else:
        big = int(np.argmax(areas))  # (the first of equals)
        R0, t0 = one_marker_pose(cam.model, cam.K, cam.D, P[4 * big:4 * big + 4], img[4 * big:4 * big + 4])
    param, _ = lev_marq([cam.alone()], np.zeros(len(P), int), P, img, np.concatenate([rotvec(R0), t0]))
    return param[:3], param[3:]


# ---------------------------------------------------------------------------------------------- the whole call on one time step
def shoelace(c) -> float:
    c = np.asarray(c, float).reshape(4, 2)
    return abs(sum(c[i][0] * c[(i + 1) % 4][1] - c[(i + 1) % 4][0] * c[i][1] for i in range(4)))


def gather(cams, entries, ids_per_cam, corners_per_cam):
    """-> (used: list of (camera, list index), n_over, n_unposable).  The cameras in index order, a frame's list in list order; ids
    the map does not name skipped; an id twice WITHIN a frame left out of that frame; an equidistant marker with a corner that cannot
    be undistorted left out and counted; the first MAX_USED survivors used."""
    named = set(int(e["id"]) for e in entries)
    used, n_unposable = [], 0
    for c, (ids, corners) in enumerate(zip(ids_per_cam, corners_per_cam)):
        ids = [int(i) for i in np.asarray(ids).reshape(-1)]
        corners = np.asarray(corners, np.float32).astype(np.float64).reshape(-1, 4, 2)
        for m, i in enumerate(ids):
            if i not in named or ids.count(i) != 1:
                continue
            if cams[c].model == cm.EQUIDISTANT and not all(undistort(cams[c].model, cams[c].K, cams[c].D, float(u), float(v))[2] for u, v in corners[m]):
                n_unposable += 1
                continue
            used.append((c, m))
    return used[:MAX_USED], max(len(used) - MAX_USED, 0), n_unposable


def restate(cams, entries, ids_per_cam, corners_per_cam, sigma_px=None) -> dict:
    """One time step: the fields of fid_rig_pose_out, plus `P`, `img`, `pcam` (the used points), `start` (the rig start, six
    parameters), `costs` (the joint solve's squared error norms, the start's first) and, with sigma_px, `cov` (status, n_points,
    sigma2, cov_rt, cov_pose, cov_cam_pose)."""
    C = len(cams)
    used, n_over, n_unposable = gather(cams, entries, ids_per_cam, corners_per_cam)
    out = dict(n_markers=len(used), n_cameras=0, n_over=0, n_unposable=0, start_camera=0, n_per_camera=np.zeros(MAX_CAMERAS, int), rvec=np.zeros(3),
               tvec=np.zeros(3), R=np.zeros((3, 3)), rig_R=np.zeros((3, 3)), rig_t=np.zeros(3), image_error=0.0, err_per_camera=np.zeros(MAX_CAMERAS))
    if sigma_px is not None:
        out["cov"] = dict(status=1, n_points=0, sigma2=0.0, cov_rt=np.zeros((6, 6)), cov_pose=np.zeros((6, 6)), cov_cam_pose=np.zeros((6, 6)))
    if not used:
        return out
    by_id = {int(e["id"]): e for e in entries}
    corners = [np.asarray(c, np.float32).astype(np.float64).reshape(-1, 4, 2) for c in corners_per_cam]
    P = np.concatenate([fid_corners(by_id[int(np.asarray(ids_per_cam[c]).reshape(-1)[m])]["len"]) @ by_id[int(np.asarray(ids_per_cam[c]).reshape(-1)[m])]["R"].T
                        + by_id[int(np.asarray(ids_per_cam[c]).reshape(-1)[m])]["t"] for c, m in used])
    img = np.concatenate([corners[c][m] for c, m in used])
    mcam = np.array([c for c, _ in used])
    pcam = np.repeat(mcam, 4)
    areas = np.array([shoelace(corners[c][m]) for c, m in used])
    n_per = np.bincount(mcam, minlength=MAX_CAMERAS)
    # ---- the start camera: the largest summed area, the lowest index of equals; its solve; the composition with its extrinsic
    best, sc = -1.0, 0
    for c in range(C):
        if n_per[c]:
            a = 0.0
            for v in areas[mcam == c]:
                a += v
            if a > best:
                best, sc = a, c
    rs, ts = solve_one_camera(cams[sc], P[pcam == sc], img[pcam == sc], areas[mcam == sc])
    R0 = cams[sc].R.T @ rodrigues(rs)
    start = np.concatenate([rotvec(R0), cams[sc].R.T @ (ts - cams[sc].t)])
    # ---- the joint solve, always
    param, costs = lev_marq(cams, pcam, P, img, start)
    R = rodrigues(param[:3])
    d = img - project(cams, pcam, param, P).astype(np.float32).astype(np.float64)
    e2 = (d * d).sum(axis=1)
    err_per = np.zeros(MAX_CAMERAS)
    for c in range(C):
        if n_per[c]:
            err_per[c] = e2[pcam == c].sum() / (4 * n_per[c])
    out.update(n_cameras=int((n_per > 0).sum()), n_over=n_over, n_unposable=n_unposable, start_camera=sc, n_per_camera=n_per, rvec=param[:3], tvec=param[3:],
               R=R, rig_R=R.T, rig_t=-R.T @ param[3:], image_error=float(e2.sum() / len(P)), err_per_camera=err_per, P=P, img=img, pcam=pcam, start=start,
               costs=costs)
    if sigma_px is not None:
        out["cov"] = covariance(cams, pcam, P, img, param, sigma_px)
    return out


def covariance(cams, pcam, P, img, param, sigma_px) -> dict:
    """fid_abi.h's "pose covariance" on the joint Jacobian at `param`: cov_rt = sigma^2 (J^T J)^-1, cov_pose = A cov_rt A^T,
    cov_cam_pose = B cov_pose B^T (the rig in the map)."""
    from pose_cov_cases import A_closed, B_closed

    uv, J = project(cams, pcam, param, P, True)
    J, e = J.reshape(-1, 6), (uv - np.asarray(img, float).reshape(-1, 2)).reshape(-1)
    n = len(uv)
    sigma2 = float(sigma_px) ** 2 if sigma_px > 0 else float(e @ e) / (2 * n - 6)
    cov_rt = sigma2 * np.linalg.inv(J.T @ J)
    cov_rt = 0.5 * (cov_rt + cov_rt.T)
    A, B = A_closed(param[:3]), B_closed(param[:3], param[3:])
    cov_pose = A @ cov_rt @ A.T
    return dict(status=0, n_points=n, sigma2=sigma2, cov_rt=cov_rt, cov_pose=cov_pose, cov_cam_pose=B @ cov_pose @ B.T, JtJ=J.T @ J)


def exact_minimum(cams, pcam, P, img, param0):
    """The minimiser of the joint reprojection error: Gauss-Newton from param0 until the step is below 1e-14."""
    p = np.array(param0, float)
    for _ in range(200):
        uv, J = project(cams, pcam, p, P, True)
        step = np.linalg.lstsq(J.reshape(-1, 6), -(uv - img).reshape(-1), rcond=None)[0]
        p = p + step
        if np.linalg.norm(step) < 1e-14:
            return p
    raise AssertionError("the Gauss-Newton reference did not converge")
