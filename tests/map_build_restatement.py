"""fid_build_map_cam and fid_map_save_file (include/fid_abi.h: "building the map") restated in NumPy, float64: the selection of a view's
markers, FEW_VIEWS and the reachability fixed point, the start rule, the residual vector, a dense Levenberg-Marquardt run to a
standstill on a complex-step Jacobian over ALL parameters, cov from the dense (J^T J)^-1, and the file line.  It is the reference of
tests/test_gpu_map_build.py; no test functions and no GPU here.

A view is (corners (n, 4, 2), ids (n,)) as detect_markers_batch returns it, or the pair the other way round.  A camera is (model, k16):
the sixteen slots fx fy cx cy D[0..11] of calib_restatement.  fixed: MAP_ENTRY_DTYPE records.  The parameter vector of the joint
problem is (rvec, t) of every free marker in the solve in id order, followed by (rvec, tvec) of every used view in view order.

The projection is camera_model_cases.distort's on a batch of observations, every observation with its own marker and view pose, real
or complex, so that one complex step reaches a parameter of every observation at once."""
from __future__ import annotations

import numpy as np

import camera_model_cases as cmc
from calib_restatement import homography_dlt, is_planar, plane_frame, rotation_vector

MAX_VIEWS, MAX_MARKERS, MAX_PER_VIEW = 4096, 128, 64
M_FIXED, M_SOLVED, M_FEW_VIEWS, M_UNREACHED, M_NO_START = range(5)
V_USED, V_FEW, V_UNREACHED, V_NO_START = range(4)
BIG_ROWS = 3000


class TooManyMarkers(Exception):
    pass


# ---------------------------------------------------------------------------------------------- selection and reachability
def split_view(view):
    a, b = view
    ids, corners = (a, b) if np.asarray(a).ndim <= 1 and np.asarray(b).ndim > 1 else (b, a)
    ids = np.asarray(ids).reshape(-1).astype(int)
    return ids, np.asarray(corners, np.float32).astype(np.float64).reshape(len(ids), 4, 2)


def keep(ids, max_per_view: int = MAX_PER_VIEW):
    """List order, an id seen twice left out altogether, the first max_per_view kept -> (list positions, n_over)."""
    ids = [int(i) for i in ids]
    pos = [m for m, i in enumerate(ids) if ids.count(i) == 1]
    return pos[:max_per_view], max(len(pos) - max_per_view, 0)


def plan(views, fixed_ids, min_views: int = 2):
    """-> dict(ids (all kept, ascending), n_views {id}, mstatus {id} (FIXED / SOLVED stand for "in the solve"), vstatus [..], kept
    [[(list position, id)]], n_over [..], solve (ids in the solve, ascending))."""
    kept, n_over = [], []
    for v in views:
        ids, _ = split_view(v)
        pos, over = keep(ids)
        kept.append([(m, int(ids[m])) for m in pos])
        n_over.append(over)
    all_ids = sorted({i for k in kept for _, i in k})
    n_views = {i: sum(1 for k in kept for _, j in k if j == i) for i in all_ids}
    fixed_ids = set(int(i) for i in fixed_ids)
    cand = {i for i in all_ids if i in fixed_ids or n_views[i] >= min_views}
    placed = {i for i in all_ids if i in fixed_ids}
    reached = [False] * len(views)
    changed = True
    while changed:
        changed = False
        for v, k in enumerate(kept):
            if not reached[v] and any(i in placed for _, i in k):
                reached[v] = changed = True
                placed |= {i for _, i in k if i in cand}
    mstatus = {}
    for i in all_ids:
        mstatus[i] = M_FIXED if i in fixed_ids else M_FEW_VIEWS if i not in cand else M_SOLVED if i in placed else M_UNREACHED
    vstatus = [V_USED if reached[v] else V_FEW if not any(i in cand for _, i in k) else V_UNREACHED for v, k in enumerate(kept)]
    solve = [i for i in all_ids if i in placed]
    if len(solve) > MAX_MARKERS:
        raise TooManyMarkers(len(solve))
    return dict(ids=all_ids, n_views=n_views, mstatus=mstatus, vstatus=vstatus, kept=kept, n_over=n_over, solve=solve)


def lengths(ids, fiducial_len, len_override, fixed):
    out = {int(i): float(fiducial_len) for i in ids}
    for i, l in (len_override or {}).items():
        if int(i) in out:
            out[int(i)] = float(l)
    for e in fixed:
        if int(e["id"]) in out:
            out[int(e["id"])] = float(e["len"])
    return out


# ---------------------------------------------------------------------------------------------- projection and residuals
def half(length) -> float:
    return float(np.float32(length / 2))


def rodrigues_b(r):
    """Rotation vectors (..., 3), real or complex -> matrices (..., 3, 3): I + sin(th) [k]x + (1 - cos(th)) [k]x^2."""
    r = np.asarray(r)
    th = np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1] + r[..., 2] * r[..., 2])
    small = np.abs(th) < np.finfo(float).eps
    ths = np.where(small, 1.0, th)
    k = r / ths[..., None]
    z = np.zeros_like(k[..., 0])
    kx = np.stack([np.stack([z, -k[..., 2], k[..., 1]], -1), np.stack([k[..., 2], z, -k[..., 0]], -1), np.stack([-k[..., 1], k[..., 0], z], -1)], -2)
    sn = np.where(small, 0.0, np.sin(ths))[..., None, None]
    c1 = np.where(small, 0.0, 1.0 - np.cos(ths))[..., None, None]
    return np.eye(3) + sn * kx + c1 * (kx @ kx)


def project_obs(model, k16, mR, mt, vr, vt, h):
    """O observations -> pixels (O, 4, 2): marker poses (mR (O, 3, 3), mt (O, 3)), view poses (vr, vt (O, 3)), half lengths h (O,)."""
    sx = np.array([-1.0, 1.0, 1.0, -1.0])
    sy = np.array([1.0, 1.0, -1.0, -1.0])
    M = np.stack([h[:, None] * sx, h[:, None] * sy, np.zeros((len(h), 4))], -1)
    pmap = np.einsum("oij,oqj->oqi", mR, M) + mt[:, None, :]
    pcam = np.einsum("oij,oqj->oqi", rodrigues_b(vr), pmap) + np.asarray(vt)[:, None, :]
    xd, yd = cmc.distort(model, list(k16[4:]), pcam[..., 0] / pcam[..., 2], pcam[..., 1] / pcam[..., 2])
    return np.stack([xd * k16[0] + k16[2], yd * k16[1] + k16[3]], -1)


class Problem:
    """One call's observations and parameters.  obs: (view index among the used views, slot among the markers in the solve, corners
    (4, 2)).  fixed_R / fixed_t: {slot: ...}; free: the free slots in order."""

    def __init__(self, model, k16, n_slots, fixed, h, obs, n_views):
        self.model, self.k16 = model, np.asarray(k16, np.float64)
        self.fixed = fixed
        self.free = [s for s in range(n_slots) if s not in fixed]
        self.col = {s: 6 * i for i, s in enumerate(self.free)}
        self.nm = 6 * len(self.free)
        self.n_views = n_views
        self.ov = np.array([o[0] for o in obs], int)
        self.os = np.array([o[1] for o in obs], int)
        self.img = np.stack([o[2] for o in obs]).astype(np.float64)
        self.h = np.array([h[s] for s in self.os])
        self.n_slots = n_slots
        self.is_free = np.array([s in self.col for s in self.os])
        self.mcol = np.array([self.col.get(s, 0) for s in self.os], int)
        self.fR = np.stack([fixed[s][0] if s in fixed else np.eye(3) for s in range(n_slots)])
        self.ft = np.stack([fixed[s][1] if s in fixed else np.zeros(3) for s in range(n_slots)])

    def n(self):
        return self.nm + 6 * self.n_views

    def pack(self, mposes, vposes):
        return np.concatenate([np.asarray(mposes[s], np.float64) for s in self.free] + [np.asarray(p, np.float64) for p in vposes])

    def _obs_params(self, x):
        mp = x[:self.nm].reshape(-1, 6)[self.mcol // 6] if self.nm else np.zeros((len(self.os), 6))
        vp = x[self.nm:].reshape(-1, 6)[self.ov]
        return mp, vp

    def _res(self, mp, vp):
        f = self.is_free[:, None, None]
        mR = np.where(f, rodrigues_b(mp[:, :3]), self.fR[self.os])
        mt = np.where(self.is_free[:, None], mp[:, 3:], self.ft[self.os])
        return project_obs(self.model, self.k16, mR, mt, vp[:, :3], vp[:, 3:], self.h) - self.img

    def res(self, x):
        """The residual vector: observations in (view, list) order, u0 v0 u1 v1 u2 v2 u3 v3 of each."""
        return self._res(*self._obs_params(x)).reshape(-1)

    def jacobian(self, x, h: float = 1e-30):
        """Complex-step Jacobian over all parameters: one step per local direction reaches every observation's own marker / view."""
        mp, vp = self._obs_params(x)
        J = np.zeros((8 * len(self.os), self.n()))
        rows = np.arange(8 * len(self.os)).reshape(-1, 8)
        for d in range(6):
            m2 = mp.astype(np.complex128)
            m2[:, d] += 1j * h
            dm = np.imag(self._res(m2, vp)).reshape(-1, 8) / h
            v2 = vp.astype(np.complex128)
            v2[:, d] += 1j * h
            dv = np.imag(self._res(mp, v2)).reshape(-1, 8) / h
            fo = np.nonzero(self.is_free)[0]
            J[rows[fo], (self.mcol[fo] + d)[:, None]] = dm[fo]
            J[rows, (self.nm + 6 * self.ov + d)[:, None]] = dv
        return J


def lm(prob, x0, max_iter: int = 500, rel_step: float = 1e-15):
    """calib_restatement.lm's dense Levenberg-Marquardt on this problem -> (x, cost, iterations)."""
    x = np.asarray(x0, np.float64).copy()
    r = prob.res(x)
    c = float(r @ r)
    lg, it = -3, 0
    while it < max_iter:
        J = prob.jacobian(x)
        s = np.sqrt((J * J).sum(axis=0))
        s[s == 0] = 1.0
        Js = J / s
        moved = False
        big = J.shape[0] > BIG_ROWS  # (the same step from the normal equations of the scaled Jacobian where the stacked solve takes seconds)
        if big:
            Hs, gs = Js.T @ Js, Js.T @ r
        while it < max_iter and lg <= 16:
            it += 1
            if big:
                step = np.linalg.solve(Hs + 10.0 ** lg * np.eye(len(x)), gs) / s
            else:
                A = np.vstack([Js, np.sqrt(10.0 ** lg) * np.eye(len(x))])
                step = np.linalg.lstsq(A, np.concatenate([r, np.zeros(len(x))]), rcond=None)[0] / s
            xn = x - step
            rn = prob.res(xn)
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


def covariance(prob, x, sigma_px: float = 0.0):
    """-> (cov {free slot: (6, 6)}, std of every parameter (for the parity bars), cost, dof): blocks of (J^T J)^-1 over the whole
    vector times cost / dof, or sigma_px^2."""
    J = prob.jacobian(x)
    r = prob.res(x)
    c = float(r @ r)
    s = np.sqrt((J * J).sum(axis=0))
    _, R = np.linalg.qr(J / s)
    Rinv = np.linalg.inv(R)
    dof = len(r) - len(x)
    f = sigma_px ** 2 if sigma_px > 0 else (c / dof if dof > 0 else 0.0)
    cov = {}
    for sl in prob.free:
        i = slice(prob.col[sl], prob.col[sl] + 6)
        cov[sl] = Rinv[i] @ Rinv[i].T / np.outer(s[i], s[i]) * f
    diag = (Rinv * Rinv).sum(axis=1) / (s * s)
    return cov, np.sqrt(diag * (c / dof if dof > 0 else 0.0)), c, dof


# ---------------------------------------------------------------------------------------------- the start
def area(corners) -> float:
    """calcFiducialArea: Heron on the two triangles of the quad."""
    c = np.asarray(corners, np.float64).reshape(4, 2)
    d = lambda a, b: float(np.hypot(*(c[a] - c[b])))
    a1, b1, c1, a2, b2 = d(0, 1), d(0, 3), d(1, 3), d(1, 2), d(2, 3)
    s1, s2 = (a1 + b1 + c1) / 2, (a2 + b2 + c1) / 2
    return float(np.sqrt(max(s1 * (s1 - a1) * (s1 - b1) * (s1 - c1), 0)) + np.sqrt(max(s2 * (s2 - a2) * (s2 - b2) * (s2 - c1), 0)))


def _pose_lm(model, k16, obj, img, pose0):
    """One pose over points in a common frame: a Problem with one fixed marker at identity per point set would do; this is the same
    machine on a single six-vector."""
    obj, img = np.asarray(obj, np.float64), np.asarray(img, np.float64)

    class One:
        def res(self, x):
            pc = obj @ cmc.rodrigues(x[:3]).T + x[3:]
            xd, yd = cmc.distort(model, list(k16[4:]), pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2])
            return (np.stack([xd * k16[0] + k16[2], yd * k16[1] + k16[3]], 1) - img).reshape(-1)

        def jacobian(self, x, h=1e-30):
            J = np.zeros((2 * len(obj), 6))
            for j in range(6):
                xc = x.astype(np.complex128)
                xc[j] += 1j * h
                J[:, j] = np.imag(self.res(xc)) / h
            return J
    return lm(One(), pose0, max_iter=100, rel_step=1e-13)[0]


def planar_pose(model, k16, obj, img):
    """The pose of coplanar points: the homography of their plane to the undistorted normalised image points, decomposed (what
    k_pose and k_map_pose start from), then the pose-only solve on the pixels."""
    obj, img = np.asarray(obj, np.float64), np.asarray(img, np.float64).reshape(-1, 2)
    Rt, tt = plane_frame(obj)
    nrm = np.array([cmc.undistort_exact(model, list(k16[4:]), (u - k16[2]) / k16[0], (v - k16[3]) / k16[1]) for u, v in img])
    G = homography_dlt((obj @ Rt.T + tt)[:, :2], nrm)
    sc = 2.0 / (np.linalg.norm(G[:, 0]) + np.linalg.norm(G[:, 1]))
    if G[2, 2] * sc < 0:
        sc = -sc
    r1, r2, t = G[:, 0] * sc, G[:, 1] * sc, G[:, 2] * sc
    U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], axis=1))
    Rp = U @ Vt  # plane frame -> camera
    return _pose_lm(model, k16, obj, img, np.concatenate([rotation_vector(Rp @ Rt), Rp @ tt + t]))


def marker_pose(model, k16, corners, length):
    """fid_pose_cam's job for one marker."""
    return planar_pose(model, k16, _corners(length), corners)


def start(model, k16, views, pl, fixed, lens):
    """The start rule -> (marker poses {id: (R, t)}, view poses {v: six})."""
    placed = {int(e["id"]): (np.asarray(e["R"], np.float64), np.asarray(e["t"], np.float64)) for e in fixed if int(e["id"]) in pl["solve"]}
    split = [split_view(v) for v in views]
    single = {}

    def one(v, m, i):
        if (v, m) not in single:
            single[(v, m)] = marker_pose(model, k16, split[v][1][m], lens[i])
        return single[(v, m)]
    vposes = {}
    changed = True
    while changed:
        changed = False
        for v, k in enumerate(pl["kept"]):
            if v in vposes or pl["vstatus"][v] != V_USED:
                continue
            have = [(m, i) for m, i in k if i in placed]
            if not have:
                continue
            obj = np.concatenate([_corners(lens[i]) @ placed[i][0].T + placed[i][1] for _, i in have])
            img = np.concatenate([split[v][1][m] for m, _ in have])
            if is_planar(obj):  # (k_map_pose's two starts: the homography over all points, or the largest marker composed with its place)
                vposes[v] = planar_pose(model, k16, obj, img)
            else:
                m0, i0 = max(have, key=lambda mi: area(split[v][1][mi[0]]))
                p = one(v, m0, i0)
                Rcf, (Rmf, tmf) = cmc.rodrigues(p[:3]), placed[i0]
                Rcm = Rcf @ Rmf.T
                vposes[v] = _pose_lm(model, k16, obj, img, np.concatenate([rotation_vector(Rcm), p[3:] - Rcm @ tmf]))
            changed = True
        for i in pl["solve"]:
            if i in placed:
                continue
            best = None
            for v in sorted(vposes):
                for m, j in pl["kept"][v]:
                    if j == i and (best is None or area(split[v][1][m]) > best[0]):
                        best = (area(split[v][1][m]), v, m)
            if best is None:
                continue
            _, v, m = best
            p = one(v, m, i)
            Rcm, Rcf = cmc.rodrigues(vposes[v][:3]), cmc.rodrigues(p[:3])
            placed[i] = (Rcm.T @ Rcf, Rcm.T @ (p[3:] - vposes[v][3:]))
            changed = True
    return placed, vposes


def _corners(length):
    h = half(length)
    return np.array([[-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0.0]])


# ---------------------------------------------------------------------------------------------- a whole call
def problem_of(model, k16, views, pl, fixed, lens):
    """The Problem of a plan: slots = pl['solve'] in order, used views = those with vstatus USED, in order."""
    slot = {i: s for s, i in enumerate(pl["solve"])}
    fx = {slot[int(e["id"])]: (np.asarray(e["R"], np.float64), np.asarray(e["t"], np.float64)) for e in fixed if int(e["id"]) in slot}
    used = [v for v, s in enumerate(pl["vstatus"]) if s == V_USED]
    obs = []
    for u, v in enumerate(used):
        _, corners = split_view(views[v])
        obs += [(u, slot[i], corners[m]) for m, i in pl["kept"][v] if i in slot]
    h = {slot[i]: half(lens[i]) for i in pl["solve"]}
    return Problem(model, k16, len(slot), fx, h, obs, len(used)), slot, used


def build(model, k16, views, fixed, fiducial_len, len_override=None, min_views: int = 2, sigma_px: float = 0.0, start_poses=None, max_iter: int = 500):
    """The reference answer of one call.  start_poses: None for the rule's start, or (marker poses {id: six}, view poses {v: six}) for
    the markers in the solve that are not fixed and the used views.  max_iter = 0 returns the start."""
    pl = plan(views, fixed["id"], min_views)
    lens = lengths(pl["ids"], fiducial_len, len_override, fixed)
    prob, slot, used = problem_of(model, k16, views, pl, fixed, lens)
    if start_poses is None:
        placed, vposes = start(model, k16, views, pl, fixed, lens)
        mstart = {slot[i]: np.concatenate([rotation_vector(placed[i][0]), placed[i][1]]) for i in pl["solve"] if slot[i] in prob.col}
        vstart = [vposes[v] for v in used]
    else:
        mstart = {slot[i]: np.asarray(start_poses[0][i], np.float64) for i in pl["solve"] if slot[i] in prob.col}
        vstart = [np.asarray(start_poses[1][v], np.float64) for v in used]
    x0 = prob.pack(mstart, vstart)
    r0 = prob.res(x0)
    x, c, it = (x0, float(r0 @ r0), 0) if max_iter == 0 else lm(prob, x0, max_iter=max_iter)
    cov, std, c2, dof = covariance(prob, x, sigma_px)
    r = prob.res(x).reshape(-1, 8)
    mrms = {i: float(np.sqrt((r[prob.os == slot[i]] ** 2).sum() / (4 * (prob.os == slot[i]).sum()))) for i in pl["solve"]}
    vrms = {v: float(np.sqrt((r[prob.ov == u] ** 2).sum() / (4 * (prob.ov == u).sum()))) for u, v in enumerate(used)}
    mposes = {i: x[prob.col[slot[i]]:prob.col[slot[i]] + 6] for i in pl["solve"] if slot[i] in prob.col}
    vposes = {v: x[prob.nm + 6 * u:prob.nm + 6 * u + 6] for u, v in enumerate(used)}
    return dict(plan=pl, lens=lens, problem=prob, slot=slot, used=used, x=x, x0=x0, cost=c, start_cost=float(r0 @ r0), iterations=it,
                cov={i: cov[slot[i]] for i in mposes}, std=std, dof=dof, rms=float(np.sqrt(c / (4 * len(prob.os)))), mrms=mrms, vrms=vrms, mposes=mposes,
                vposes=vposes, n_points=4 * len(prob.os), n_free=prob.n())


# ---------------------------------------------------------------------------------------------- the file line
def rpy_deg(R):
    R = np.asarray(R, np.float64)
    if abs(R[2, 0]) >= 1:
        pitch = np.pi / 2 if R[2, 0] < 0 else -np.pi / 2
        roll = np.arctan2(R[0, 1], R[0, 2]) if R[2, 0] < 0 else np.arctan2(-R[0, 1], -R[0, 2])
        yaw = 0.0
    else:
        pitch, roll, yaw = np.arcsin(-R[2, 0]), np.arctan2(R[2, 1], R[2, 2]), np.arctan2(R[1, 0], R[0, 0])
    return np.degrees([roll, pitch, yaw])


def file_line(id_, R, t, variance, n_obs, links) -> str:
    """map.cpp:556-562: "%d %lf %lf %lf %lf %lf %lf %lf %d" and " %d" per link."""
    r = rpy_deg(R)
    return "%d %f %f %f %f %f %f %f %d" % (id_, t[0], t[1], t[2], r[0], r[1], r[2], variance, n_obs) + "".join(" %d" % l for l in sorted(links)) + "\n"
