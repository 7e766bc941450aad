"""fid_calibrate_map (include/fid_abi.h: "camera calibration from views of the map") restated in NumPy, float64: the selection of a
view's markers, the AUTO start, the residual vector, a dense Levenberg-Marquardt run to a standstill on a complex-step Jacobian over
ALL parameters, and std_dev.  It is the reference of tests/test_gpu_calibrate.py; no test functions and no GPU here.

A view is (ids (n,), corners (n, 4, 2)), or the pair the other way round as detect_markers_batch returns it.  The sixteen slots are fx fy cx cy D[0..11]; a camera is the vector k16 of them.  The
parameter vector of the joint problem is the free slots in ascending order (with fix_aspect: fy stands for both, fx = aspect fy)
followed by (rvec, tvec) of every used view in view order.

The projection is camera_model_cases.project's, built on the same rodrigues / distort, with K and D allowed to be complex so that
the complex step reaches the intrinsics as well."""
from __future__ import annotations

import numpy as np

import camera_model_cases as cmc
from aruco_map_cases import fid_corners

MAX_USED = 256
SLOTS = 16


# ---------------------------------------------------------------------------------------------- selection
def select(map_ids, view_ids, max_used: int = MAX_USED):
    """fid_map_pose_cam's selection -> (list positions of the used markers, n_over)."""
    mapped = set(int(i) for i in map_ids)
    view_ids = [int(i) for i in view_ids]
    count = {}
    for i in view_ids:
        count[i] = count.get(i, 0) + 1
    pos = [m for m, i in enumerate(view_ids) if i in mapped and count[i] == 1]
    return pos[:max_used], max(len(pos) - max_used, 0)


def view_points(entries, view):
    """(object points (4 n, 3), image points (4 n, 2) float64, n_over) of the used markers of one view."""
    a, b = view  # (ids, corners) or, as detect_markers_batch returns them, (corners, ids): the ids are the flat one
    ids, corners = (a, b) if np.asarray(a).ndim <= 1 and np.asarray(b).ndim > 1 else (b, a)
    ids = np.asarray(ids).reshape(-1)
    corners = np.asarray(corners).reshape(len(ids), 4, 2)
    by_id = {int(e["id"]): e for e in entries}
    pos, n_over = select(entries["id"], ids)
    if not pos:
        return np.zeros((0, 3)), np.zeros((0, 2)), n_over
    obj = np.concatenate([fid_corners(by_id[int(ids[m])]["len"]) @ by_id[int(ids[m])]["R"].T + by_id[int(ids[m])]["t"] for m in pos])
    img = np.concatenate([np.asarray(corners[m], np.float32).astype(np.float64).reshape(4, 2) for m in pos])
    return obj, img, n_over


# ---------------------------------------------------------------------------------------------- projection and residuals
def project(model: int, k16, rvec, tvec, pts):
    """Object points -> pixels; k16, rvec, tvec real or complex."""
    k16 = np.asarray(k16)
    pcam = np.asarray(pts, dtype=np.float64) @ cmc.rodrigues(np.asarray(rvec)).T + np.asarray(tvec)
    xd, yd = cmc.distort(model, list(k16[4:]), pcam[:, 0] / pcam[:, 2], pcam[:, 1] / pcam[:, 2])
    return np.stack([xd * k16[0] + k16[2], yd * k16[1] + k16[3]], axis=1)


def residuals(model: int, k16, poses, points):
    """The residual vector (u0 v0 u1 v1 ... per view, views in order): projection minus corner.  points: [(obj, img)] per used view."""
    return np.concatenate([(project(model, k16, p[:3], p[3:], obj) - img).reshape(-1) for p, (obj, img) in zip(poses, points)])


def cost(model: int, k16, poses, points) -> float:
    r = residuals(model, k16, poses, points)
    return float(r @ r)


class Problem:
    """The free parameters of one call: which slots, fix_aspect, the fixed values."""

    def __init__(self, model: int, k16, free_mask: int, fix_aspect: bool = False):
        self.model = model
        self.k0 = np.asarray(k16, dtype=np.float64).copy()
        mask = free_mask & ~1 if fix_aspect else free_mask
        self.cols = [i for i in range(SLOTS) if mask >> i & 1]
        self.fix_aspect = bool(fix_aspect) and bool(mask >> 1 & 1)
        self.aspect = self.k0[0] / self.k0[1] if fix_aspect else 1.0
        self.nI = len(self.cols)

    def k16(self, x):
        k = self.k0.astype(np.result_type(self.k0, x))
        k[self.cols] = x[:self.nI]
        if self.fix_aspect:
            k[0] = self.aspect * k[1]
        return k

    def pack(self, k16, poses):
        return np.concatenate([np.asarray(k16, dtype=np.float64)[self.cols]] + [np.asarray(p, dtype=np.float64) for p in poses])

    def unpack(self, x):
        return self.k16(x), x[self.nI:].reshape(-1, 6)

    def res(self, x, points):
        k, poses = self.unpack(x)
        return residuals(self.model, k, poses, points)

    def jacobian(self, x, points, h: float = 1e-30):
        """Complex-step Jacobian over all parameters (each view's rows depend on the intrinsics and on its own six only)."""
        nI, nres = self.nI, sum(2 * len(o) for o, _ in points)
        J = np.zeros((nres, len(x)))
        r0 = 0
        for v, (obj, img) in enumerate(points):
            rows = slice(r0, r0 + 2 * len(obj))
            for j in list(range(nI)) + list(range(nI + 6 * v, nI + 6 * v + 6)):
                xc = x.astype(np.complex128)
                xc[j] += 1j * h
                k, poses = self.unpack(xc)
                J[rows, j] = np.imag(project(self.model, k, poses[v][:3], poses[v][3:], obj)).reshape(-1) / h
            r0 += 2 * len(obj)
        return J


def lm(prob: Problem, x0, points, max_iter: int = 500, rel_step: float = 1e-15):
    """Dense Levenberg-Marquardt (lambda in powers of ten from 1e-3, the damped matrix J^T J with its diagonal times 1 + lambda, accept
    on a cost that does not rise) run until it stands still: a relative step below rel_step or lambda past 1e16.  The damped step is
    solved as a least-squares problem on the column-scaled Jacobian, which is the same step with a better-conditioned solve.
    -> (x, cost, iterations)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    r = prob.res(x, points)
    c = float(r @ r)
    lg = -3
    it = 0
    while it < max_iter:
        J = prob.jacobian(x, points)
        s = np.sqrt((J * J).sum(axis=0))
        s[s == 0] = 1.0
        Js = J / s
        moved = False
        while it < max_iter and lg <= 16:
            it += 1
            lam = 10.0 ** lg
            A = np.vstack([Js, np.sqrt(lam) * np.eye(len(x))])
            b = np.concatenate([r, np.zeros(len(x))])
            step = np.linalg.lstsq(A, b, rcond=None)[0] / s
            xn = x - step
            rn = prob.res(xn, points)
            cn = float(rn @ rn)
            if np.isfinite(cn) and cn <= c:
                rel = np.linalg.norm(step) / (np.linalg.norm(x) + np.finfo(float).eps)
                x, r, c = xn, rn, cn
                lg = max(lg - 1, -16)
                moved = True
                if rel < rel_step:
                    return x, c, it
                break
            lg += 1
        if not moved:
            break
    return x, c, it


def std_dev(prob: Problem, x, points):
    """(std_dev[16], rms): sqrt(diag((J^T J)^-1) cost / (2 N - n_free)) over the whole parameter vector, scattered to the slots."""
    J = prob.jacobian(x, points)
    r = prob.res(x, points)
    c = float(r @ r)
    s = np.sqrt((J * J).sum(axis=0))
    Js = J / s
    _, R = np.linalg.qr(Js)
    Rinv = np.linalg.inv(R)
    d = (Rinv * Rinv).sum(axis=1) / (s * s)  # diag((J^T J)^-1)
    dof = len(r) - len(x)
    sd = np.zeros(SLOTS)
    if dof > 0:
        sd[prob.cols] = np.sqrt(d[:prob.nI] * c / dof)
        if prob.fix_aspect:
            sd[0] = abs(prob.aspect) * sd[1]
    return sd, float(np.sqrt(c / (len(r) // 2)))


# ---------------------------------------------------------------------------------------------- the AUTO start
def plane_frame(obj):
    """The frame of a coplanar set: rotation whose rows are the scatter matrix's eigenvectors (descending), right-handed; origin at
    the centroid.  -> (Rt, tt) with plane coordinates Rt X + tt."""
    mc = obj.mean(axis=0)
    w, V = np.linalg.eigh((obj - mc).T @ (obj - mc))
    Rt = V[:, ::-1].T.copy()
    if Rt[0, 2] ** 2 + Rt[1, 2] ** 2 < 1e-10:
        Rt = np.eye(3)
    if np.linalg.det(Rt) < 0:
        Rt = -Rt
    return Rt, -Rt @ mc


def is_planar(obj) -> bool:
    mc = obj.mean(axis=0)
    w = np.sort(np.linalg.eigvalsh((obj - mc).T @ (obj - mc)))[::-1]
    return bool(w[2] / w[1] < 1e-3)


def homography_dlt(XY, uv):
    """findHomography's normalised DLT, H[2][2] = 1."""
    def norm(p):
        c = p.mean(axis=0)
        s = len(p) / np.abs(p - c).sum(axis=0)
        return (p - c) * s, c, s
    P, cP, sP = norm(XY)
    m, cm, sm = norm(uv)
    L = []
    for (X, Y), (x, y) in zip(P, m):
        L.append([X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x])
        L.append([0, 0, 0, X, Y, 1, -y * X, -y * Y, -y])
    L = np.asarray(L)
    w, V = np.linalg.eigh(L.T @ L)
    H0 = V[:, 0].reshape(3, 3)
    inv_m = np.array([[1 / sm[0], 0, cm[0]], [0, 1 / sm[1], cm[1]], [0, 0, 1]])
    nP = np.array([[sP[0], 0, -cP[0] * sP[0]], [0, sP[1], -cP[1] * sP[1]], [0, 0, 1]])
    H = inv_m @ H0 @ nP
    return H / H[2, 2]


def auto_start(model: int, k16, free_mask: int, fix_aspect: bool, points, image_size):
    """fid_abi.h's START_AUTO -> (k16 of the start, [pose per view]).  The per-view poses come from the homography under the start
    camera's focal lengths and principal point, refined by this module's own pose-only solve (the device takes fid_map_pose_cam's)."""
    w, h = image_size
    k = np.asarray(k16, dtype=np.float64).copy()
    mask = free_mask & ~1 if fix_aspect else free_mask
    cx = (w - 1) / 2 if mask >> 2 & 1 else k[2]
    cy = (h - 1) / 2 if mask >> 3 & 1 else k[3]
    rows, rhs, Hs = [], [], []
    for obj, img in points:
        if not is_planar(obj):
            raise ValueError("START_AUTO needs coplanar views")
        Rt, tt = plane_frame(obj)
        XY = (obj @ Rt.T + tt)[:, :2].astype(np.float32).astype(np.float64)
        H = homography_dlt(XY, img)
        Hs.append((H.copy(), Rt, tt))
        H[0] -= H[2] * cx
        H[1] -= H[2] * cy
        h1, h2 = H[:, 0], H[:, 1]
        d1, d2 = (h1 + h2) / 2, (h1 - h2) / 2
        h1, h2, d1, d2 = (q / np.linalg.norm(q) for q in (h1, h2, d1, d2))
        rows += [[h1[0] * h2[0], h1[1] * h2[1]], [d1[0] * d2[0], d1[1] * d2[1]]]
        rhs += [-h1[2] * h2[2], -d1[2] * d2[2]]
    X, Y = np.linalg.lstsq(np.asarray(rows), np.asarray(rhs), rcond=None)[0]
    fx, fy = np.sqrt(abs(1 / X)), np.sqrt(abs(1 / Y))
    aspect = k[0] / k[1]
    if mask >> 1 & 1:
        k[1] = fy
    if mask & 1:
        k[0] = fx
    k[2], k[3] = cx, cy
    for i in range(12):
        if mask >> (4 + i) & 1:
            k[4 + i] = 0.0
    if fix_aspect and mask >> 1 & 1:
        k[0] = aspect * k[1]
    poses = []
    Kinv = np.linalg.inv(np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]]))
    for (H, Rt, tt), (obj, img) in zip(Hs, points):
        G = Kinv @ H
        sc = 2.0 / (np.linalg.norm(G[:, 0]) + np.linalg.norm(G[:, 1]))
        if G[2, 2] * sc < 0:
            sc = -sc
        r1, r2, t = G[:, 0] * sc, G[:, 1] * sc, G[:, 2] * sc
        U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], axis=1))
        Rp = U @ Vt  # plane frame -> camera
        R = Rp @ Rt
        tv = Rp @ tt + t
        pose0 = np.concatenate([rotation_vector(R), tv])
        one = Problem(model, k, 0)
        x, _, _ = lm(one, pose0, [(obj, img)], max_iter=60, rel_step=1e-12)
        poses.append(x)
    return k, poses


def rotation_vector(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    n = np.linalg.norm(ax)
    if n < 1e-12:
        return np.array([1e-9, 0.0, 0.0]) if th < 1 else np.pi * np.sqrt(np.maximum((np.diag(R) + 1) / 2, 0))
    return ax / n * th


# ---------------------------------------------------------------------------------------------- a whole call
def calibrate(entries, views, image_size, model: int, k16, free_mask: int, fix_aspect: bool = False, start: str = "auto", min_markers: int = 1,
              start_poses=None):
    """The reference answer of one call -> dict(k16, poses, cost, rms, std_dev, used (view indices), n_points, iterations).
    start = "auto", or "given" with start_poses (one per USED view; None: the AUTO poses under the given camera)."""
    pts_all = [view_points(entries, v) for v in views]
    used = [i for i, (o, _, _) in enumerate(pts_all) if len(o) >= 4 * max(min_markers, 1)]
    points = [(pts_all[i][0], pts_all[i][1]) for i in used]
    if start == "auto":
        k0, poses0 = auto_start(model, k16, free_mask, fix_aspect, points, image_size)
    else:
        k0 = np.asarray(k16, dtype=np.float64).copy()
        poses0 = start_poses if start_poses is not None else auto_start(model, k0, 0, False, points, image_size)[1]
    prob = Problem(model, k0, free_mask, fix_aspect)
    if fix_aspect:
        prob.aspect = float(k16[0]) / float(k16[1])
    x, c, it = lm(prob, prob.pack(prob.k16(prob.pack(k0, [])), poses0), points)
    sd, rms = std_dev(prob, x, points)
    k, poses = prob.unpack(x)
    return dict(k16=k, poses=poses, cost=c, rms=rms, std_dev=sd, used=used, n_points=sum(len(o) for o, _ in points), iterations=it, problem=prob,
                points=points, x=x)
