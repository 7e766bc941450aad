"""The NumPy statement of the pose covariance (pose_cov_cases.py) held to itself, without a device: the closed forms A and B of
include/fid_abi.h against central differences of log(R' R^T), and the predicted cov_pose against the scatter of poses refined from
noisy corners (Monte Carlo)."""
import numpy as np
import pytest

import camera_model_cases as cm
import pose_cases as pc
import pose_cov_cases as cc

DRAWS = 3000
SIGMA = 0.02


def _all_poses():
    out = []
    for set_name in cc.CAMERA_SETS:
        _, _, _, _, Rs, ts = cc.marker_cases(set_name)
        out += [(cc.rvec_of(R), t) for R, t in zip(Rs, ts)]
    out += [(cc.rvec_of(R), t) for R, t in zip(*cc.stag_cases()[2:])]
    out += [(cc.rvec_of(R), t) for _, _, R, t in cc.bundle_cases()[1]]
    out.append((cc.rvec_of(cc.map_case()[4]), cc.map_case()[5]))
    return out


def test_closed_forms_agree_with_central_differences():
    """A = [[0, I], [J_l, 0]] and B = [[-R^T, -R^T [t]x], [0, -R^T]] against the five-point central differences, on every pose of the
    device test and on rotation vectors below the series threshold: 1e-10 (the stencil at h = 1e-3 is good to ~1e-12; a wrong sign
    or a right-Jacobian in J_l's place moves an entry by 1e-1)."""
    worst_a = worst_b = 0.0
    for rvec, tvec in _all_poses() + [(np.array([3e-5, -2e-5, 4e-5]), np.array([0.1, -0.2, 1.5])), (np.array([1e-7, 0.0, 0.0]), np.array([0.3, 0.1, 0.9]))]:
        worst_a = max(worst_a, float(np.abs(cc.A_closed(rvec) - cc.A_numeric(rvec)).max()))
        worst_b = max(worst_b, float(np.abs(cc.B_closed(rvec, tvec) - cc.B_numeric(rvec, tvec)).max()))
    print(f"\nclosed forms against central differences: A {worst_a:.3g}, B {worst_b:.3g}")
    assert worst_a <= 1e-10 and worst_b <= 1e-10


def test_whitened_dev_and_the_two_inverses():
    S = np.diag([1.0, 4.0, 9.0])
    assert cc.whitened_dev(S, S) < 1e-15
    assert abs(cc.whitened_dev(1.01 * S, S) - 0.01) < 1e-12
    assert 0.0 < cc.cpu_disagreement() and cc.tol() <= cc.TOL_CAP


def _gauss_newton(model, K, D, rvec, tvec, obj, img):
    p = np.concatenate([rvec, tvec])
    for _ in range(6):
        J = cm.complex_step_jacobian(model, K, D, p[:3], p[3:], obj).reshape(-1, 6)
        e = (cm.project(model, K, D, p[:3], p[3:], obj) - img).reshape(-1)
        step = np.linalg.solve(J.T @ J, J.T @ e)
        p = p - step
        if np.abs(step).max() < 1e-13:
            break
    return p


@pytest.mark.parametrize("set_name", ["barrel", "prism12"])
def test_monte_carlo_scatter_matches_cov_pose(set_name):
    """Side 80 px, tilt 45 degrees (the fourth marker of the cases), sigma 0.02 px, 3 000 draws with a fixed seed, each refined by
    Gauss-Newton on the complex-step Jacobian from the generating pose.  The poses' deviations from the generating pose as (dt,
    log(R_i R^T)), their sample covariance whitened by the predicted cov_pose: every diagonal within 5 sqrt(2 / (n - 1)) of 1 and
    every off-diagonal within the same bound of 0 -- five standard deviations of a chi-square sample variance, derived and not tuned."""
    model, D = cc.CAMERA_SETS[set_name]
    K = pc.camera_matrix(cc.CAM)
    _, _, _, objs, Rs, ts = cc.marker_cases(set_name)
    obj, R0, t0 = objs[3], Rs[3], ts[3]
    assert cc.MARKERS[3][2:] == (80.0, 45.0)
    r0 = cc.rvec_of(R0)
    img0 = cm.project(model, K, D, r0, t0, obj)
    _, cov_pose, sigma2 = cc.reference_cov(model, K, D, r0, t0, obj, img0, SIGMA)
    assert sigma2 == SIGMA ** 2
    rng = np.random.default_rng(20261018)
    X = np.zeros((DRAWS, 6))
    for i in range(DRAWS):
        p = _gauss_newton(model, K, D, r0, t0, obj, img0 + SIGMA * rng.standard_normal(img0.shape))
        X[i, :3] = p[3:] - t0
        X[i, 3:] = cc.so3_log(pc.rodrigues(p[:3]) @ R0.T)
    S = np.cov(X.T)
    Li = np.linalg.inv(np.linalg.cholesky(cov_pose))
    Wm = Li @ S @ Li.T
    bound = 5.0 * np.sqrt(2.0 / (DRAWS - 1))
    off = Wm - np.diag(np.diag(Wm))
    print(f"\n{set_name}: whitened sample covariance diagonal {np.diag(Wm).min():.3f} .. {np.diag(Wm).max():.3f}, largest off-diagonal {np.abs(off).max():.3f}; bound {bound:.3f}")
    assert np.abs(np.diag(Wm) - 1.0).max() <= bound
    assert np.abs(off).max() <= bound
