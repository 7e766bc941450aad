"""The consensus map pose (fid_abi.h: "map pose that survives wrong markers") restated in NumPy from the header's text: the used
markers, eligibility, err, the one-marker hypotheses (undistort, Heckbert's quad homography, the pose from it, composed with the
marker's place in the map), the lower median, the first set and the rounds.  No test functions and no GPU.

The solve of a round is not restated: it is oracle.solve_pnp_points where the set is plumb-bob, coplanar and has <= 32 points (the
oracle's range), else the exact minimiser of the same reprojection error started from the winning hypothesis (Gauss-Newton to a step
below 1e-14; for plumb-bob stag_bundle_cases.exact_minimiser, for the other models the same iteration on camera_model_cases'
complex-step Jacobian).  The two differ from CvLevMarq's stopping point by ~1e-9 (aruco_map_cases.oracle_gap_to_minimum), which no
decision of a kept case can feel: map_robust_cases keeps a case only if every err clears its threshold by more than 1 %."""
from __future__ import annotations

import numpy as np

import camera_model_cases as cm
from stag_bundle_cases import exact_minimiser

MAX_USED, HYPOTHESES, SOLVES = 256, 64, 4
OK, NO_CONSENSUS, NO_MARKERS = 0, 1, 2
FISHEYE_MAX_THETA = np.deg2rad(89.0)


def fid_corners(length: float) -> np.ndarray:
    h = float(np.float32(length / 2))
    return np.array([[-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0]])


def undistort(model: int, K, D, u: float, v: float):
    """Pixel -> normalised pinhole point and whether the model can do it.  Plumb-bob, rational: five fixed-point iterations, always
    possible.  Equidistant: Newton on theta from theta_d (ten steps at most, until the step is below 1e-8); impossible where that
    has not converged or theta is outside [0, 89 degrees)."""
    k = list(D) + [0.0] * (12 - len(D))
    x = x0 = (u - K[0, 2]) / K[0, 0]
    y = y0 = (v - K[1, 2]) / K[1, 1]
    if model == cm.EQUIDISTANT:
        thd = float(np.hypot(x, y))
        th, ok = thd, False
        for _ in range(10):
            th2 = th * th
            f = th * (1 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3])))) - thd
            df = 1 + th2 * (3 * k[0] + th2 * (5 * k[1] + th2 * (7 * k[2] + th2 * 9 * k[3])))
            th -= f / df
            if abs(f / df) < 1e-8:
                ok = True
                break
        ok = ok and 0.0 <= th < FISHEYE_MAX_THETA
        sc = np.tan(th) / thd if (ok and thd > 1e-8) else 1.0
        return x * sc, y * sc, ok
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        if model == cm.RATIONAL:
            icd *= 1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        if model == cm.RATIONAL:
            dx += k[8] * r2 + k[9] * r2 * r2
            dy += k[10] * r2 + k[11] * r2 * r2
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y, True


def quad_homography(q: np.ndarray) -> np.ndarray:
    """Heckbert: the homography that takes the unit square (0,0), (1,0), (1,1), (0,1) to the quad q (4, 2)."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = q
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dy1 * dx2
    g, h = (sx * dy2 - sy * dx2) / den, (dx1 * sy - dy1 * sx) / den
    return np.array([[x1 - x0 + g * x1, x3 - x0 + h * x3, x0], [y1 - y0 + g * y1, y3 - y0 + h * y3, y0], [g, h, 1.0]])


def _nearest_rotation(M: np.ndarray) -> np.ndarray:
    U, _, Vt = np.linalg.svd(M)  # (cv::Rodrigues of a matrix: R = U V^T)
    return U @ Vt


def one_marker_pose(model: int, K, D, obj4: np.ndarray, img4: np.ndarray):
    """h_k: the closed-form pose of one marker (its four map points obj4 and image corners img4) in the MAP's frame.  The marker's
    frame: x along corner 0 -> 1, y along corner 3 -> 0, origin at the middle of corners 0 and 2."""
    ex, ey = obj4[1] - obj4[0], obj4[0] - obj4[3]
    wx, wy = np.linalg.norm(ex), np.linalg.norm(ey)
    ex = ex / wx
    ez = np.cross(ex, ey)
    ez /= np.linalg.norm(ez)
    ey = np.cross(ez, ex)
    cc = 0.5 * (obj4[0] + obj4[2])
    mn = np.array([undistort(model, K, D, float(u), float(v))[:2] for u, v in img4])
    # marker plane (X, Y) -> unit square (X / wx + 1/2, 1/2 - Y / wy) -> quad
    H = quad_homography(mn) @ np.array([[1 / wx, 0, 0.5], [0, -1 / wy, 0.5], [0, 0, 1.0]])
    H = H / H[2, 2]
    n1, n2 = np.linalg.norm(H[:, 0]), np.linalg.norm(H[:, 1])
    tq = H[:, 2] * 2.0 / (n1 + n2)
    r1, r2 = H[:, 0] / n1, H[:, 1] / n2
    Rq = _nearest_rotation(np.stack([r1, r2, np.cross(r1, r2)], axis=1))
    R = Rq @ np.stack([ex, ey, ez])  # map -> camera: Rq B^T (X - cc) + tq
    return R, tq - R @ cc


def err(model: int, K, D, R, t, obj4, img4) -> float:
    d = cm.project(model, K, D, R, t, obj4) - img4
    return float(np.sqrt((d * d).sum(axis=1)).max())


def _rotvec(R: np.ndarray) -> np.ndarray:
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    s, c = np.linalg.norm(w), (np.trace(R) - 1) / 2
    th = np.arctan2(s, c)
    return w * (th / s) if s > 1e-12 else w


def _minimise_any(model: int, K, D, P, img, R0, t0):
    """Gauss-Newton on (rvec, tvec) with the complex-step Jacobian until the step is below 1e-14."""
    if model == cm.PLUMB_BOB:
        return exact_minimiser(P, img, R0, t0, K, np.asarray(list(D) + [0.0] * 5, float)[:5])
    r, t = _rotvec(R0), np.array(t0, float)
    for _ in range(500):
        res = (cm.project(model, K, D, r, t, P) - img).reshape(-1)
        J = cm.complex_step_jacobian(model, K, D, r, t, P).reshape(-1, 6)
        step = np.linalg.lstsq(J, -res, rcond=None)[0]
        r, t = r + step[:3], t + step[3:]
        if np.linalg.norm(step) < 1e-14:
            return cm.rodrigues(r), t
    raise AssertionError("the Gauss-Newton reference did not converge")


def _coplanar(P: np.ndarray) -> bool:
    d = P - P.mean(axis=0)
    w = np.sort(np.linalg.eigvalsh(d.T @ d))[::-1]
    return w[2] / w[1] < 1e-3


def solve(model: int, K, D, P, img, R0, t0):
    if model == cm.PLUMB_BOB and len(P) <= 32 and _coplanar(P):
        import oracle
        r, tv = oracle.solve_pnp_points(K, np.asarray(list(D) + [0.0] * 5, float)[:5], P, img)
        return cm.rodrigues(r) if np.linalg.norm(r) > 0 else np.eye(3), tv
    return _minimise_any(model, K, D, P, img, R0, t0)


def used_markers(map_ids, ids):
    """(list indices of the used markers in list order, n_over)"""
    named = set(int(i) for i in map_ids)
    ids = [int(i) for i in ids]
    used = [m for m, i in enumerate(ids) if i in named and ids.count(i) == 1]
    return used[:MAX_USED], max(len(used) - MAX_USED, 0)


def restate(model: int, K, D, entries, ids, corners, inlier_px: float, min_markers: int, winner=None, hypotheses: int = HYPOTHESES) -> dict:
    """The whole call on one frame.  entries: MAP_ENTRY_DTYPE; ids (n,), corners (n, 4, 2) float32 in list order.  Returns the
    record's content plus what the case filter needs: `decisions`, every (err, threshold) pair that was compared, and `scores`.
    winner (a used index) overrides the choice of k*, hypotheses the number of them: what-if questions of the case filter."""
    K = np.asarray(K, float).reshape(3, 3)
    corners = np.asarray(corners, np.float32).astype(np.float64).reshape(-1, 4, 2)
    by_id = {int(e["id"]): e for e in entries}
    used, n_over = used_markers(by_id.keys(), ids)
    out = dict(status=NO_MARKERS, used=used, n_over=n_over, inliers=[], hypothesis=-1, rounds=0, stable=0, score=-1.0, R=None, t=None, I0=[],
               decisions=[], scores={}, eligible=[])
    if not used:
        return out
    obj = [fid_corners(by_id[int(ids[m])]["len"]) @ by_id[int(ids[m])]["R"].T + by_id[int(ids[m])]["t"] for m in used]
    img = [corners[m] for m in used]
    n = len(used)
    elig = [k for k in range(n) if all(undistort(model, K, D, float(u), float(v))[2] for u, v in img[k])]
    out["eligible"] = elig
    out["status"] = NO_CONSENSUS
    if not elig:
        return out

    def area(k):
        c = img[k]
        return abs(sum(c[i][0] * c[(i + 1) % 4][1] - c[(i + 1) % 4][0] * c[i][1] for i in range(4)))

    hyp = sorted(elig, key=lambda k: (-area(k), k))[:hypotheses]
    poses, scores = {}, {}
    for k in hyp:
        poses[k] = one_marker_pose(model, K, D, obj[k], img[k])
        e = sorted(err(model, K, D, *poses[k], obj[j], img[j]) for j in elig)
        scores[k] = e[(len(e) - 1) // 2]
    win = min(hyp, key=lambda k: (scores[k], k)) if winner is None else winner
    out.update(hypothesis=used[win], score=scores[win], scores=scores)
    thr0 = max(inlier_px, 3 * scores[win])

    def admit(R, t, thr):
        keep = []
        for j in elig:
            e = err(model, K, D, R, t, obj[j], img[j])
            out["decisions"].append((e, thr))
            if e <= thr:
                keep.append(j)
        return keep

    I = admit(*poses[win], thr0)
    out["I0"] = list(I)
    R, t = poses[win]
    while len(I) >= min_markers:
        R, t = solve(model, K, D, np.concatenate([obj[j] for j in I]), np.concatenate([img[j] for j in I]), R, t)
        out["rounds"] += 1
        nxt = admit(R, t, inlier_px)
        if nxt == I:
            out.update(status=OK, stable=1)
            break
        if len(nxt) < min_markers:
            I = []
            break
        if out["rounds"] == SOLVES:
            out.update(status=OK)
            break
        I = nxt
    if out["status"] == OK:
        out.update(inliers=I, R=R, t=t)
        out["errs"] = {j: err(model, K, D, R, t, obj[j], img[j]) for j in elig}
    return out
