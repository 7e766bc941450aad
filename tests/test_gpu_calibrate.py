"""fid_calibrate_map on the device against the NumPy restatement (tests/calib_restatement.py) on the cases of tests/calib_cases.py.

THE BARS (none chosen from what the device gives).  With t = max(10 x the reference's own two-start cost gap of the case, 1e-9):
  cost        the device's answer, evaluated by the restatement's residual function, costs at most the reference minimum x (1 + t)
  parameters  under the quadratic model a point whose cost exceeds the minimum by the fraction t lies within sqrt(2 t dof) standard
              deviations in every parameter; the bar is 2 sqrt(2 t dof) std_dev_ref per slot (the 2: the model is quadratic only roughly)
  std_dev     relative, at most max(10 x the reference's two-start gap in std_dev, 1e-6); rms likewise with its own gap
The factor ten is the one the robust map pose's threshold took over its measured value.

MEASURED ON THE MI355X: every bar holds with room (calib_cases.DEVICE_MEASURED).  The weakest case, rational k1 k2 k4 over 3 views x 6
markers, is a valley of the cost (k1 = -4.17, k4 = -4.19, std_dev of fx 33 px) in which the minimiser moves by 1e-7 .. 1e-6 standard
deviations with every rounding the residual function makes differently: the reference's own answer moves by 3.6e-7 standard
deviations, and its std_dev by 4.7e-7, when its projection multiplies by 1 / z instead of dividing by z.  That is why the device's
residual function follows the restatement's arithmetic expression by expression (fid_calib.hip, cal_rotation_value / cal_pinhole /
cal_distort); with cvProjectPoints2's expressions instead, this case's std_dev read 1.43e-6 against its bar of 1e-6."""
import ctypes as C

import numpy as np
import pytest

import calib_cases as cc
import calib_restatement as cr
from fiducials_amd import _lib, camera
from fiducials_amd.detector import ArucoDetector

pytestmark = pytest.mark.gpu

MARKER_DT = np.dtype([("id", "<i4"), ("corners", "<f4", (8,))])
N_DIST = {0: 5, 1: 8, 2: 4}
MAX_ITER = 3000  # (the weakest case takes the reference 200 iterations; a trial is four small launches)
EPS = 1e-15      # the reference's own standstill (calib_restatement.lm's rel_step), not the header's default
WORST = {"cost": 0.0, "param": 0.0, "std": 0.0, "rms": 0.0}


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(dictionary=6, max_width=640, max_height=480, max_batch=8, max_markers=64)
    yield d
    d.close()


def pack_views(views):
    views = [(np.asarray(c, np.float32).reshape(-1, 8), np.asarray(i, np.int32).reshape(-1)) for c, i in views]
    cap = max([len(i) for _, i in views] + [1])
    mk = np.zeros((len(views), cap), MARKER_DT)
    n = np.zeros(len(views), np.int32)
    for v, (c, i) in enumerate(views):
        n[v] = len(i)
        mk["id"][v, :len(i)] = i
        mk["corners"][v, :len(i)] = c
    return mk, n, cap


def cam_of(model, k16, n_dist=None):
    k16 = np.asarray(k16, dtype=np.float64)
    nd = N_DIST[model] if n_dist is None else n_dist
    return camera.Camera(model, [[k16[0], 0, k16[2]], [0, k16[1], k16[3]], [0, 0, 1]], k16[4:4 + nd])


def k16_of_cam(cam) -> np.ndarray:
    c = cam.c
    return np.array([c.K[0], c.K[4], c.K[2], c.K[5]] + list(c.D[:12]))


def calibrate(det, views, image_size, cam, free, start=_lib.CALIB_START_AUTO, fix_aspect=0, max_iter=MAX_ITER, eps=None, min_markers=1, packed=None):
    """fid_calibrate_map as it is -> (status, Camera, out record, views array)"""
    L = det._L
    mk, n, cap = packed if packed is not None else pack_views(views)
    opts = _lib.FidCalibOpts()
    L.fid_default_calib_opts(C.byref(opts))
    opts.free_mask, opts.start, opts.fix_aspect, opts.max_iter, opts.min_markers = free, start, fix_aspect, max_iter, min_markers
    opts.eps = EPS if eps is None else eps
    cam = camera.Camera(cam.model, cam.K, cam.D)
    out = np.zeros(1, _lib.CALIB_OUT_DTYPE)
    vout = np.zeros(len(n), _lib.CALIB_VIEW_DTYPE)
    rc = L.fid_calibrate_map(det._ctx, mk.ctypes.data, n.ctypes.data, len(n), cap, image_size[0], image_size[1], C.byref(opts), C.byref(cam.c),
                             out.ctypes.data, vout.ctypes.data)
    return rc, cam, out[0], vout


def hold_to_reference(c, ref, cam, out, vout, label):
    """The four bars of the module docstring, the figures printed first."""
    best = ref["best"]
    used = [v for v in range(len(vout)) if vout["status"][v] == _lib.CALIB_VIEW_USED]
    assert used == best["used"], (used, best["used"])
    k_dev = k16_of_cam(cam)
    poses_dev = [np.concatenate([vout["rvec"][v], vout["tvec"][v]]) for v in used]
    cost_dev = cr.cost(c["model"], k_dev, poses_dev, best["points"])
    t = max(10.0 * ref["gap"], 1e-9)
    dof = 2 * best["n_points"] - len(best["x"])
    free = [i for i in range(16) if c["free"] >> i & 1]
    excess = cost_dev / best["cost"] - 1.0
    z = np.abs(k_dev[free] - best["k16"][free]) / (2.0 * np.sqrt(2.0 * t * dof) * best["std_dev"][free])
    bar_std, bar_rms = max(10.0 * ref["gap_std"], 1e-6), max(10.0 * ref["gap_rms"], 1e-6)
    d_std = float(np.max(np.abs(out["std_dev"][free] - best["std_dev"][free]) / best["std_dev"][free]))
    d_rms = abs(out["rms"] - best["rms"]) / best["rms"]
    sd_here, _ = cr.std_dev(best["problem"], best["problem"].pack(k_dev, poses_dev), best["points"])  # (the restatement AT the device's answer)
    print(f"{label}: std_dev against the restatement's at the device's own answer {np.max(np.abs(out['std_dev'][free] - sd_here[free]) / sd_here[free]):.3e}")
    print(f"{label}: status {out['status']} trials {out['n_iter']} cost excess {excess:.3e} (bar {t:.1e}) parameters {z.max():.3e} of the bar "
          f"std_dev {d_std:.3e} (bar {bar_std:.1e}) rms {d_rms:.3e} (bar {bar_rms:.1e}) reported cost vs restatement {out['cost'] / cost_dev - 1:.1e}")
    for key, val in (("cost", excess / t), ("param", z.max()), ("std", d_std / bar_std), ("rms", d_rms / bar_rms)):
        WORST[key] = max(WORST[key], float(val))
    assert out["n_points"] == best["n_points"] and out["n_views_used"] == len(used) and out["n_free"] == len(best["x"])
    assert cost_dev <= best["cost"] * (1.0 + t)
    assert out["cost"] <= out["start_cost"]
    assert z.max() <= 1.0
    assert d_std <= bar_std
    assert d_rms <= bar_rms
    fixed = [i for i in range(16) if i not in free]
    assert (k_dev[fixed] == cc.zero_start(c)[fixed]).all()


@pytest.mark.parametrize("model_name,shape", cc.CASES)
def test_parity_with_the_reference(det, model_name, shape):
    c, ref = cc.case(model_name, shape), cc.reference(model_name, shape)
    assert ref["kept"]
    det.set_map(c["entries"])
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], cc.zero_start(c), c["n_dist"]), c["free"])
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    hold_to_reference(c, ref, cam, out, vout, f"{model_name} {shape}")


def test_views_of_64_65_256_and_257_markers(det):
    c, ref = cc.sizes_case(), cc.sizes_reference()
    det.set_map(c["entries"])
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], cc.zero_start(c)), c["free"])
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    assert list(vout["n_used"]) == [64, 65, 256, 256] and list(vout["n_over"]) == [0, 0, 0, 1]
    hold_to_reference(c, ref, cam, out, vout, "sizes")


def test_views_that_are_skipped_and_markers_that_are_left_out(det):
    c, ref = cc.mixed_case(), cc.mixed_reference()
    det.set_map(c["entries"])
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], cc.zero_start(c)), c["free"], min_markers=3)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    assert list(vout["status"]) == [0, _lib.CALIB_VIEW_FEW, _lib.CALIB_VIEW_FEW, 0, 0, 0]
    assert list(vout["n_used"]) == [12, 0, 2, 11, 12, 12]
    assert (vout["rvec"][1] == 0).all() and vout["rms"][2] == 0
    hold_to_reference(c, ref, cam, out, vout, "mixed")


def test_rational_with_all_eight_free_runs_and_the_cost_does_not_rise(det):
    c = cc.case(*cc.RATIONAL8)
    det.set_map(c["entries"])
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], cc.zero_start(c), 8), c["free"], max_iter=200)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    print("rational, eight free: status", out["status"], "trials", out["n_iter"], "cost", out["start_cost"], "->", out["cost"], "rms", out["rms"])
    assert np.isfinite(out["cost"]) and out["cost"] <= out["start_cost"]


def _two_walls():
    from aruco_map_cases import K as K_MAP, corner_of_two_walls, look_at, object_points, project
    entries = corner_of_two_walls(6, 6)
    P = object_points(entries)
    rng = np.random.default_rng(77)
    views, poses = [], []
    for i in range(6):
        R, t = look_at(np.array([0.9 + 0.1 * i, 0.15 * (i - 2), 1.0 - 0.08 * i]), np.array([0.2, 0.1, 0.2]))
        uv = project(P, R, t, K_MAP, np.zeros(5)) + 0.2 * rng.standard_normal((len(P), 2))
        views.append((uv.astype(np.float32).reshape(-1, 4, 2), entries["id"].astype(np.int32)))
        poses.append(np.concatenate([cr.rotation_vector(R), t]))
    k16 = np.zeros(16)
    k16[:4] = K_MAP[0, 0], K_MAP[1, 1], K_MAP[0, 2], K_MAP[1, 2]
    return entries, views, poses, k16


def test_two_wall_map_takes_a_given_start_and_refuses_auto(det):
    entries, views, poses, k16 = _two_walls()
    det.set_map(entries)
    start = k16.copy()
    start[:4] *= (1.05, 0.96, 1.02, 0.97)
    free = _lib.CALIB_FREE_K | 1 << 4
    rc, cam, out, vout = calibrate(det, views, (640, 480), cam_of(0, start), free, start=_lib.CALIB_START_GIVEN)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    pts = [cr.view_points(entries, v)[:2] for v in views]
    prob = cr.Problem(0, k16, free)
    x, cost, _ = cr.lm(prob, prob.pack(k16, poses), pts)
    k_dev = k16_of_cam(cam)
    cost_dev = cr.cost(0, k_dev, [np.concatenate([vout["rvec"][v], vout["tvec"][v]]) for v in range(len(views))], pts)
    sd, _ = cr.std_dev(prob, x, pts)
    dof = 2 * out["n_points"] - len(x)
    z = np.abs(k_dev[prob.cols] - prob.k16(x)[prob.cols]) / (2 * np.sqrt(2 * 1e-9 * dof) * sd[prob.cols])
    print(f"two walls: trials {out['n_iter']} cost excess {cost_dev / cost - 1:.3e} parameters {z.max():.3e} of the bar")
    assert cost_dev <= cost * (1 + 1e-9) and z.max() <= 1.0
    rc, _, _, _ = calibrate(det, views, (640, 480), cam_of(0, start), free, start=_lib.CALIB_START_AUTO)
    assert rc == _lib.FID_E_INVALID_ARG
    assert b"coplanar" in det._L.fid_last_error(det._ctx)


@pytest.mark.parametrize("copies", [4, 16, 64])
def test_large_calls_of_copies_of_a_16_view_case(det, copies):
    """The replicated problem has the 16-view problem's stationarity equations times a constant: its minimiser is the 16-view
    reference's, and std_dev shrinks by what the formula gives: sqrt((2 N - n_free) / (copies (2 N - n_free) + (copies - 1) nI)) / sqrt(copies)
    -- J^T J's intrinsics complement grows by `copies`, the cost by `copies`, the degrees of freedom as written."""
    c, ref = cc.case(*cc.LARGE_BASE), cc.reference(*cc.LARGE_BASE)
    assert ref["kept"]
    best = ref["best"]
    det.set_map(c["entries"])
    rc, cam, out, vout = calibrate(det, c["views"] * copies, c["image_size"], cam_of(c["model"], cc.zero_start(c)), c["free"])
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    assert out["n_views_used"] == 16 * copies and out["n_points"] == copies * best["n_points"]
    t = max(10.0 * ref["gap"], 1e-9)
    free = [i for i in range(16) if c["free"] >> i & 1]
    dof1 = 2 * best["n_points"] - len(best["x"])
    dofc = 2 * out["n_points"] - out["n_free"]
    k_dev = k16_of_cam(cam)
    z = np.abs(k_dev[free] - best["k16"][free]) / (2.0 * np.sqrt(2.0 * t * dof1) * best["std_dev"][free])
    sd_expected = best["std_dev"][free] * np.sqrt(dof1 / dofc)
    d_std = float(np.max(np.abs(out["std_dev"][free] - sd_expected) / sd_expected))
    d_rms = abs(out["rms"] - best["rms"]) / best["rms"]
    print(f"{16 * copies} views: status {out['status']} trials {out['n_iter']} parameters {z.max():.3e} of the bar std_dev {d_std:.3e} rms {d_rms:.3e}")
    assert z.max() <= 1.0
    assert d_std <= max(10.0 * ref["gap_std"], 1e-6) and d_rms <= max(10.0 * ref["gap_rms"], 1e-6)
    assert (vout["rvec"][:16] == vout["rvec"][16 * (copies - 1):]).all()  # (copies of a view get the same pose, to the bit)


def test_masks(det):
    c = cc.case("plumb_bob", "12x12")
    det.set_map(c["entries"])
    start = c["k16"].copy()
    start[:4] *= (1.04, 1.04, 0.99, 1.01)
    start[8] = 0.0  # k3 fixed at 0 although the generating camera has -0.02: "plumb-bob without k3"
    given = cam_of(0, start)
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], given, _lib.CALIB_FREE_PLUMB_BOB_NO_K3, start=_lib.CALIB_START_GIVEN)
    assert rc == _lib.FID_OK
    k = k16_of_cam(cam)
    assert k[8] == 0.0 and out["std_dev"][8] == 0.0 and (out["std_dev"][:8] > 0).all() and (out["std_dev"][9:] == 0).all()
    pts = [cr.view_points(c["entries"], v)[:2] for v in c["views"]]
    prob = cr.Problem(0, start, _lib.CALIB_FREE_PLUMB_BOB_NO_K3)
    x, cost, _ = cr.lm(prob, prob.pack(start, c["poses"]), pts)
    cost_dev = cr.cost(0, k, [np.concatenate([vout["rvec"][v], vout["tvec"][v]]) for v in range(len(pts))], pts)
    print(f"without k3: cost excess {cost_dev / cost - 1:.3e}")
    assert cost_dev <= cost * (1 + 1e-9)
    # fixed slots byte for byte: only the focal lengths free
    odd = start.copy()
    odd[2:9] = (651.123456789, 349.987654321, -0.31, 0.11, 0.0007, -0.0011, -0.019)
    rc, cam, out, _ = calibrate(det, c["views"], c["image_size"], cam_of(0, odd), _lib.CALIB_FREE_FOCAL, start=_lib.CALIB_START_GIVEN)
    assert rc == _lib.FID_OK
    k = k16_of_cam(cam)
    assert k[2:].tobytes() == odd[2:].tobytes() and (k[:2] != odd[:2]).all()
    # fix_aspect: fx / fy stays the start's ratio
    rc, cam, out, _ = calibrate(det, c["views"], c["image_size"], given, _lib.CALIB_FREE_PLUMB_BOB, start=_lib.CALIB_START_GIVEN, fix_aspect=1)
    assert rc == _lib.FID_OK
    k = k16_of_cam(cam)
    a = start[0] / start[1]
    assert k[0] == a * k[1] and out["std_dev"][0] == abs(a) * out["std_dev"][1] and out["n_free"] == 8 + 6 * 12
    ref = cr.calibrate(c["entries"], c["views"], c["image_size"], 0, start, _lib.CALIB_FREE_PLUMB_BOB, fix_aspect=True, start="given", start_poses=c["poses"])
    print(f"fix_aspect: fy {k[1]} reference {ref['k16'][1]}")
    assert abs(k[1] - ref["k16"][1]) <= 2 * np.sqrt(2 * 1e-9 * (2 * out["n_points"] - out["n_free"])) * ref["std_dev"][1]
    # the fisheye with k3 and k4 fixed at 0
    e = cc.case("equidistant", "12x12")
    det.set_map(e["entries"])
    s = e["k16"].copy()
    s[6:8] = 0.0
    rc, cam, out, _ = calibrate(det, e["views"], e["image_size"], cam_of(2, s), 0x003F, start=_lib.CALIB_START_GIVEN)
    assert rc == _lib.FID_OK
    k = k16_of_cam(cam)
    assert (k[6:] == 0).all() and (out["std_dev"][6:] == 0).all() and out["cost"] <= out["start_cost"]


def test_refusals(det):
    c = cc.case("plumb_bob", "3x6")
    det.set_map(c["entries"])
    cam = cam_of(0, c["k16"])
    one = [(c["views"][0][0][:1], c["views"][0][1][:1])]
    rc, cam2, _, _ = calibrate(det, one, c["image_size"], cam, _lib.CALIB_FREE_PLUMB_BOB, start=_lib.CALIB_START_GIVEN)  # 8 residuals, 15 free
    assert rc == _lib.FID_E_INVALID_ARG and b"residuals" in det._L.fid_last_error(det._ctx)
    assert bytes(cam2.c) == bytes(cam.c)
    assert calibrate(det, c["views"], c["image_size"], cam, 1 << 9)[0] == _lib.FID_E_INVALID_ARG  # k4 of a plumb-bob camera
    assert calibrate(det, c["views"], c["image_size"], cam_of(2, c["k16"]), 1 << 8)[0] == _lib.FID_E_INVALID_ARG  # a fifth fisheye coefficient
    assert calibrate(det, c["views"], c["image_size"], cam, 0x1FF, start=2)[0] == _lib.FID_E_INVALID_ARG
    assert calibrate(det, c["views"], c["image_size"], cam, 0x1FF, eps=float("nan"))[0] == _lib.FID_E_INVALID_ARG
    assert calibrate(det, c["views"], c["image_size"], cam, 0x1FF, min_markers=0)[0] == _lib.FID_E_INVALID_ARG
    assert calibrate(det, c["views"], (0, 720), cam, 0x1FF)[0] == _lib.FID_E_INVALID_ARG
    bad = [(v[0].copy(), v[1]) for v in c["views"]]
    bad[1][0][2, 1, 0] = np.inf
    assert calibrate(det, bad, c["image_size"], cam, 0x1FF)[0] == _lib.FID_E_INVALID_ARG
    assert b"not finite" in det._L.fid_last_error(det._ctx)
    lost = [(v[0], v[1] + 900) for v in c["views"]]
    assert calibrate(det, lost, c["image_size"], cam, 0x1FF)[0] == _lib.FID_E_INVALID_ARG  # no view names a mapped marker
    mk, n, cap = pack_views(c["views"])
    assert calibrate(det, None, c["image_size"], cam, 0x1FF, packed=(np.zeros((1025, 1), MARKER_DT), np.zeros(1025, np.int32), 1))[0] == _lib.FID_E_INVALID_ARG
    det.set_map(None)
    assert calibrate(det, c["views"], c["image_size"], cam, 0x1FF)[0] == _lib.FID_E_INVALID_ARG
    assert b"no map" in det._L.fid_last_error(det._ctx)


# (model case, free mask, n_dist, coefficients of the start): between them every column of the Jacobian.  The rational model's numerator
# and denominator are probed apart -- with both free the problem is degenerate (calib_cases' docstring) and J^T J has no factor.
PROBES = {
    "plumb_bob": ("plumb_bob", 0x01FF, 5, None),
    "equidistant": ("equidistant", 0x00FF, 4, None),
    "rational_numerator": ("rational_k124", 0x01FF, 8, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004)),
    "rational_denominator": ("rational_k124", 0x000F | 0x0E00 | 0x00C0, 8, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004)),
    "rational_prism": ("rational_k124", 0x000F | 0xF000 | 0x0030, 12, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004, 0.0009, -0.0004, -0.0007, 0.0003)),
}


@pytest.mark.parametrize("probe", list(PROBES))
def test_the_start_s_cost_and_std_dev_against_the_complex_step_jacobian(det, probe):
    """max_iter = 0 returns the start: its cost, and std_dev from the device's analytic Jacobian (fx fy cx cy, the model's coefficients,
    the six of every pose) at the start, held to the restatement's complex-step Jacobian at the same point."""
    model_name, free, n_dist, coeffs = PROBES[probe]
    c = dict(cc.case(model_name, "12x12"), n_dist=n_dist)
    det.set_map(c["entries"])
    start = c["k16"].copy()
    start[:4] *= (1.01, 0.99, 1.005, 0.995)
    if coeffs is not None:
        start[4:4 + len(coeffs)] = coeffs
    model_name = probe
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], start, c["n_dist"]), free, start=_lib.CALIB_START_GIVEN, max_iter=0)
    assert rc == _lib.FID_OK and out["status"] == _lib.CALIB_MAX_ITER and out["n_iter"] == 0
    assert bytes(cam.c) == bytes(cam_of(c["model"], start, c["n_dist"]).c)
    pts = [cr.view_points(c["entries"], v)[:2] for v in c["views"]]
    poses = [np.concatenate([vout["rvec"][v], vout["tvec"][v]]) for v in range(len(pts))]
    prob = cr.Problem(c["model"], start, free)
    x = prob.pack(start, poses)
    sd, rms = cr.std_dev(prob, x, pts)
    cost = cr.cost(c["model"], start, poses, pts)
    fr = [i for i in range(16) if free >> i & 1]
    d = float(np.max(np.abs(out["std_dev"][fr] - sd[fr]) / sd[fr]))
    print(model_name, "std_dev", out["std_dev"][fr], "restatement", sd[fr])
    print(f"{model_name}: start cost {out['cost']} vs {cost} ({out['cost'] / cost - 1:.1e}); std_dev vs complex step {d:.3e}")
    # float64 on both sides; the inverse amplifies rounding by the conditioning of J^T J (1e9 .. 1e11 here): 1e-6 is the floor of the
    # std_dev bar above
    assert abs(out["cost"] / cost - 1) <= 1e-12 and out["start_cost"] == out["cost"]
    assert d <= 1e-6
    assert (out["std_dev"][[i for i in range(16) if i not in fr]] == 0).all()


def test_same_bytes_every_time_and_the_other_calls_untouched(det):
    from aruco_map_cases import scene, scene_map, K as K_MAP
    frames = np.stack([scene("3x2", p).image for p in range(3)])
    det.set_map(scene_map("3x2"))
    mcam = camera.Camera(0, K_MAP, np.zeros(5))
    det_before = det.detect_markers_batch(frames)
    pose_before = det.map_pose_last(camera=mcam).tobytes()
    c = cc.case("plumb_bob", "12x12")
    det.set_map(c["entries"])
    cam0 = cam_of(0, cc.zero_start(c))
    r1 = calibrate(det, c["views"], c["image_size"], cam0, c["free"])
    r2 = calibrate(det, c["views"], c["image_size"], cam0, c["free"])
    assert r1[0] == _lib.FID_OK
    same = lambda a, b: bytes(a[1].c) == bytes(b[1].c) and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert same(r1, r2)
    det.set_map(scene_map("3x2"))
    det_after = det.detect_markers_batch(frames)
    pose_after = det.map_pose_last(camera=mcam).tobytes()
    assert pose_after == pose_before
    for (ca, ia), (cb, ib) in zip(det_before, det_after):
        assert ca.tobytes() == cb.tobytes() and ia.tobytes() == ib.tobytes()
    det.set_map(c["entries"])
    r3 = calibrate(det, c["views"], c["image_size"], cam0, c["free"])
    assert same(r1, r3)


def test_end_to_end_from_rendered_views(det):
    """Eight rendered 640 x 480 views of one board -> detect_markers_batch -> calibrate_map (plumb-bob, fx fy cx cy k1 free, AUTO).
    The answer is held to the restatement on the SAME detected corners; the distance from the rendering camera is printed only
    (nobody has measured what the corner bias of rendering and detection does to it)."""
    from aruco_map_cases import FACING, K as K_MAP, grid_board
    from fiducials_amd import synth
    from fiducials_amd.dictionary import get_predefined_dictionary
    entries = grid_board(6, 3, first_id=20, length=0.08, pitch=0.13)
    det.set_map(entries)
    frames = []
    for i in range(8):
        a = 0.12 + 0.07 * i
        R = synth._rodrigues(np.array([a * np.cos(0.8 * i), a * np.sin(0.8 * i), 0.0])) @ synth._rodrigues(np.array([0.0, 0.0, 0.4 * i])) @ FACING
        t = np.array([0.03 * (i % 3 - 1), 0.02 * (i % 2) - 0.05, 0.55 + 0.04 * i])
        frames.append(synth.make_aruco_board_frame(get_predefined_dictionary(6), entries["id"], [(float(e["len"]), e["R"], e["t"]) for e in entries], K_MAP,
                                                   R, t, 100 + i, 640, 480).image)
    views = det.detect_markers_batch(np.stack(frames))
    assert all(len(ids) >= 4 for _, ids in views), [len(ids) for _, ids in views]
    free = _lib.CALIB_FREE_K | 1 << 4
    cam, out, vout = det.calibrate_map(views, (640, 480), model=_lib.CAM_PLUMB_BOB, free=free, max_iter=MAX_ITER, eps=EPS)
    k16 = np.zeros(16)
    k16[:4] = K_MAP[0, 0], K_MAP[1, 1], K_MAP[0, 2], K_MAP[1, 2]
    c = dict(model=0, k16=k16, free=free, entries=entries, views=views, poses=None, image_size=(640, 480))
    ref = cc.reference_of(c)
    assert ref["kept"], ref["gap"]
    hold_to_reference(c, ref, cam, out, vout, "end to end")
    k = k16_of_cam(cam)
    print(f"end to end: rms {out['rms']:.4f} px; from the rendering camera: fx {k[0] - k16[0]:+.3f} fy {k[1] - k16[1]:+.3f} cx {k[2] - k16[2]:+.3f} "
          f"cy {k[3] - k16[3]:+.3f} px, k1 {k[4]:+.5f}")


def test_zz_print_the_largest_figures():
    print("largest over this run, in units of their bars:", WORST)
