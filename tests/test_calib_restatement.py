"""The calibration reference (tests/calib_restatement.py) checked against itself and the cases' keep rule, and the parts of the
calibration ABI that need no device: exported symbols, struct sizes, fid_camera_to_info, the refusals."""
import ctypes as C

import numpy as np
import pytest

import calib_cases as cc
import calib_restatement as cr
from fiducials_amd import _lib, camera


@pytest.mark.parametrize("model_name,shape", cc.CASES)
def test_every_committed_case_passes_the_keep_rule(model_name, shape):
    r = cc.reference(model_name, shape)
    print(f"{model_name} {shape}: cost gap {r['gap']:.2e}, std_dev gap {r['gap_std']:.2e}, rms gap {r['gap_rms']:.2e}, "
          f"iterations {r['auto']['iterations']} / {r['given']['iterations']}")
    assert r["gap"] <= cc.KEEP_GAP
    assert r["auto"]["used"] == list(range(len(cc.case(model_name, shape)["views"])))


@pytest.mark.parametrize("model_name", list(cc.MODELS))
def test_the_generating_camera_comes_back_from_noise_free_views(model_name):
    c, r = cc.case(model_name, "5x20_exact"), cc.reference(model_name, "5x20_exact")["best"]
    free = [i for i in range(16) if c["free"] >> i & 1]
    # float32 rounding of the corners is the only noise: an rms of its size, and every free slot within a few of ITS standard deviations
    assert r["rms"] < 2.0 ** -14
    z = np.abs(r["k16"][free] - c["k16"][free]) / r["std_dev"][free]
    print(model_name, "rms", r["rms"], "worst slot, in standard deviations:", z.max(), "focal", r["k16"][:2])
    assert z.max() < 6.0
    assert abs(r["k16"][0] / cc.FX - 1) < 1e-5 and abs(r["k16"][1] / cc.FY - 1) < 1e-5
    fixed = [i for i in range(16) if i not in free]
    assert (r["k16"][fixed] == c["k16"][fixed]).all()


def test_agrees_with_scipy_where_it_is_installed():
    opt = pytest.importorskip("scipy.optimize")
    c, r = cc.case("plumb_bob", "3x6"), cc.reference("plumb_bob", "3x6")
    best = r["best"]
    prob, pts = best["problem"], best["points"]
    x0 = prob.pack(c["k16"], c["poses"])
    sol = opt.least_squares(lambda x: prob.res(x, pts), x0, jac=lambda x: prob.jacobian(x, pts), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    gap = abs(2 * sol.cost - best["cost"]) / best["cost"]
    print("scipy cost", 2 * sol.cost, "restatement", best["cost"], "gap", gap)
    assert gap <= cc.KEEP_GAP


@pytest.mark.parametrize("model_name", list(cc.MODELS))
def test_jacobian_and_std_dev_are_self_consistent(model_name):
    best = cc.reference(model_name, "3x6")["best"]
    prob, pts, x = best["problem"], best["points"], best["x"]
    J = prob.jacobian(x, pts)
    # central differences, step relative to the parameter: O(h^2) truncation + rounding / h
    for j in range(len(x)):
        h = 1e-6 * max(abs(x[j]), 1e-2)
        e = np.zeros(len(x))
        e[j] = h
        fd = (prob.res(x + e, pts) - prob.res(x - e, pts)) / (2 * h)
        assert np.abs(fd - J[:, j]).max() <= 1e-6 * max(np.abs(J[:, j]).max(), 1.0), j
    # the gradient vanishes at the minimum (against the size of its terms)
    assert np.abs(J.T @ prob.res(x, pts)).max() <= 1e-6 * (np.abs(J).T @ np.abs(prob.res(x, pts))).max()
    sd, rms = cr.std_dev(prob, x, pts)
    cov = np.linalg.inv(J.T @ J) * best["cost"] / (J.shape[0] - J.shape[1])
    np.testing.assert_allclose(sd[prob.cols], np.sqrt(np.diag(cov)[:prob.nI]), rtol=1e-5)
    assert rms == pytest.approx(np.sqrt(best["cost"] / best["n_points"]), rel=1e-14)


def test_selection_is_fid_map_pose_cam_s():
    assert cr.select([1, 2, 3, 5], [9, 2, 3, 2, 5, 7]) == ([2, 4], 0)  # 9 and 7 unmapped, 2 twice: out altogether
    pos, over = cr.select(range(300), range(300))
    assert pos == list(range(256)) and over == 44


def test_fix_aspect_ties_fx_to_fy():
    c = cc.case("plumb_bob", "3x6")
    r = cr.calibrate(c["entries"], c["views"], c["image_size"], c["model"], c["k16"], c["free"], fix_aspect=True, start="given", start_poses=c["poses"])
    assert r["k16"][0] / r["k16"][1] == pytest.approx(cc.FX / cc.FY, rel=1e-15)
    assert r["std_dev"][0] == pytest.approx(cc.FX / cc.FY * r["std_dev"][1], rel=1e-15)
    assert r["problem"].nI == 8


# ---------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_the_calibration_symbols():
    L = _lib.load()
    for name in ("fid_default_calib_opts", "fid_calibrate_map", "fid_camera_to_info"):
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS


def test_struct_sizes_match_the_mirrors():
    # fid_calib_opts: 6 x int32 + double; fid_calib_out: 6 x int32 + 3 doubles + 16 doubles; fid_calib_view: 4 x int32 + 7 doubles
    assert C.sizeof(_lib.FidCalibOpts) == 32
    assert _lib.CALIB_OUT_DTYPE.itemsize == 24 + 8 * 19
    assert _lib.CALIB_VIEW_DTYPE.itemsize == 16 + 8 * 7


def test_default_options():
    L = _lib.load()
    o = _lib.FidCalibOpts()
    L.fid_default_calib_opts(C.byref(o))
    assert (o.free_mask, o.start, o.fix_aspect, o.min_markers, o.max_iter) == (_lib.CALIB_FREE_PLUMB_BOB, _lib.CALIB_START_AUTO, 0, 1, 100)
    assert o.eps == 1e-12
    L.fid_default_calib_opts(None)  # (ignored)


@pytest.mark.parametrize("name,n_in,n_out", [("plumb_bob", 5, 5), ("plumb_bob", 4, 5), ("rational_polynomial", 8, 8), ("rational_polynomial", 12, 12),
                                             ("equidistant", 4, 4)])
def test_camera_to_info_round_trips(name, n_in, n_out):
    K = [[910.0, 0.0, 652.3], [0.0, 905.0, 348.9], [0.0, 0.0, 1.0]]
    D = [0.01 * (i + 1) * (-1) ** i for i in range(n_in)]
    cam = camera.from_info(name, K, D)
    model, K2, D2 = cam.to_info()
    assert model == name and len(D2) == n_out
    assert (K2 == np.asarray(K)).all()
    assert (D2[:n_in] == np.asarray(D)).all() and (D2[n_in:] == 0).all()
    back = camera.from_info(model, K2, D2)
    assert back.model == cam.model and (back.K == cam.K).all() and (back.D[:n_in] == cam.D).all()


def test_refusals_that_need_no_device():
    L = _lib.load()
    cam = camera.Camera(_lib.CAM_PLUMB_BOB, np.eye(3), np.zeros(5))
    name, K, D, n = C.create_string_buffer(32), (C.c_double * 9)(), (C.c_double * 12)(), C.c_int32()
    assert L.fid_camera_to_info(None, name, K, D, C.byref(n)) == _lib.FID_E_INVALID_ARG
    assert L.fid_camera_to_info(C.byref(cam.c), None, K, D, C.byref(n)) == _lib.FID_E_INVALID_ARG
    assert L.fid_camera_to_info(C.byref(cam.c), name, K, D, None) == _lib.FID_E_INVALID_ARG
    bad = camera.Camera(7, np.eye(3), np.zeros(5))
    assert L.fid_camera_to_info(C.byref(bad.c), name, K, D, C.byref(n)) == _lib.FID_E_INVALID_ARG
    opts = _lib.FidCalibOpts()
    L.fid_default_calib_opts(C.byref(opts))
    out = np.zeros(1, _lib.CALIB_OUT_DTYPE)
    mk = np.zeros(4, np.dtype([("id", "<i4"), ("corners", "<f4", (8,))]))
    nn = np.array([4], np.int32)
    assert L.fid_calibrate_map(None, mk.ctypes.data, nn.ctypes.data, 1, 4, 640, 480, C.byref(opts), C.byref(cam.c), out.ctypes.data, None) == _lib.FID_E_INVALID_ARG
