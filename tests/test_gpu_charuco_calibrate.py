"""fid_calibrate_charuco on the device against the NumPy restatement (tests/charuco_calib_restatement.py) on the cases of
tests/charuco_calib_cases.py.

THE BARS are those of tests/test_gpu_calibrate.py, copied, none chosen from what the device gives.  With t = max(10 x the reference's
own two-start cost gap of the case, 1e-9):
  cost        the device's answer, evaluated by the restatement's residual function, costs at most the reference minimum x (1 + t)
  parameters  under the quadratic model a point whose cost exceeds the minimum by the fraction t lies within sqrt(2 t dof) standard
              deviations in every parameter; the bar is 2 sqrt(2 t dof) std_dev_ref per slot (the 2: the model is quadratic only roughly)
  std_dev     relative, at most max(10 x the reference's two-start gap in std_dev, 1e-6); rms likewise with its own gap

MEASURED ON THE MI355X: charuco_calib_cases.DEVICE_MEASURED."""
import ctypes as C

import numpy as np
import pytest

import calib_cases as cc
import calib_restatement as cr
import charuco_calib_cases as ccc
import charuco_calib_restatement as ccr
from fiducials_amd import _lib, camera
from fiducials_amd.detector import ArucoDetector, FidError

pytestmark = pytest.mark.gpu

N_DIST = {0: 5, 1: 8, 2: 4}
MAX_ITER = 3000  # (the weakest case takes the reference 500 iterations; a trial is four small launches)
EPS = 1e-15      # the reference's own standstill (calib_restatement.lm's rel_step), not the header's default
WORST = {"cost": 0.0, "param": 0.0, "std": 0.0, "rms": 0.0}


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(dictionary=ccc.DICT, max_width=640, max_height=480, max_batch=8, max_markers=64)
    yield d
    d.close()


def pack_views(views):
    views = [(np.asarray(i, np.int32).reshape(-1), np.asarray(xy, np.float32).reshape(-1, 2)) for i, xy in views]
    cap = max([len(i) for i, _ in views] + [1])
    rec = np.zeros((len(views), cap), _lib.CHARUCO_CORNER_DTYPE)
    n = np.zeros(len(views), np.int32)
    for v, (i, xy) in enumerate(views):
        n[v] = len(i)
        rec["id"][v, :len(i)] = i
        rec["x"][v, :len(i)], rec["y"][v, :len(i)] = xy[:, 0], xy[:, 1]
        rec["x0"][v, :len(i)], rec["y0"][v, :len(i)], rec["win"][v, :len(i)] = np.nan, np.nan, -7  # (ignored by the call)
    return rec, n, cap


def cam_of(model, k16, n_dist=None):
    k16 = np.asarray(k16, dtype=np.float64)
    nd = N_DIST[model] if n_dist is None else n_dist
    return camera.Camera(model, [[k16[0], 0, k16[2]], [0, k16[1], k16[3]], [0, 0, 1]], k16[4:4 + nd])


def k16_of_cam(cam) -> np.ndarray:
    c = cam.c
    return np.array([c.K[0], c.K[4], c.K[2], c.K[5]] + list(c.D[:12]))


def calibrate(det, views, image_size, cam, free, start=_lib.CALIB_START_AUTO, fix_aspect=0, max_iter=MAX_ITER, eps=None, min_markers=1, packed=None):
    """fid_calibrate_charuco as it is -> (status, Camera, out record, views array)"""
    L = det._L
    rec, n, cap = packed if packed is not None else pack_views(views)
    opts = _lib.FidCalibOpts()
    L.fid_default_calib_opts(C.byref(opts))
    opts.free_mask, opts.start, opts.fix_aspect, opts.max_iter, opts.min_markers = free, start, fix_aspect, max_iter, min_markers
    opts.eps = EPS if eps is None else eps
    cam = camera.Camera(cam.model, cam.K, cam.D)
    out = np.zeros(1, _lib.CALIB_OUT_DTYPE)
    vout = np.zeros(len(n), _lib.CALIB_VIEW_DTYPE)
    rc = L.fid_calibrate_charuco(det._ctx, rec.ctypes.data, n.ctypes.data, len(n), cap, image_size[0], image_size[1], C.byref(opts), C.byref(cam.c),
                                 out.ctypes.data, vout.ctypes.data)
    return rc, cam, out[0], vout


def poses_of(vout, used):
    return [np.concatenate([vout["rvec"][v], vout["tvec"][v]]) for v in used]


def hold_to_reference(c, ref, cam, out, vout, label):
    """The four bars of the module docstring, the figures printed first."""
    best = ref["best"]
    used = [v for v in range(len(vout)) if vout["status"][v] == _lib.CALIB_VIEW_USED]
    assert used == best["used"], (used, best["used"])
    assert list(vout["status"]) == best["statuses"] and list(vout["n_used"]) == best["n_used"] and (vout["n_over"] == 0).all()
    k_dev = k16_of_cam(cam)
    poses_dev = poses_of(vout, used)
    cost_dev = cr.cost(c["model"], k_dev, poses_dev, best["points"])
    t = max(10.0 * ref["gap"], 1e-9)
    dof = 2 * best["n_points"] - len(best["x"])
    free = [i for i in range(16) if c["free"] >> i & 1]
    excess = cost_dev / best["cost"] - 1.0
    z = np.abs(k_dev[free] - best["k16"][free]) / (2.0 * np.sqrt(2.0 * t * dof) * best["std_dev"][free])
    bar_std, bar_rms = max(10.0 * ref["gap_std"], 1e-6), max(10.0 * ref["gap_rms"], 1e-6)
    d_std = float(np.max(np.abs(out["std_dev"][free] - best["std_dev"][free]) / best["std_dev"][free]))
    d_rms = abs(out["rms"] - best["rms"]) / best["rms"]
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
    assert k_dev[fixed].tobytes() == cc.zero_start(c)[fixed].tobytes()
    # the records of the views: a used view's rms over its own points, a skipped view's record zero but for status and n_used
    for v in range(len(vout)):
        if v in used:
            obj, img = best["points"][used.index(v)]
            rms_v = np.sqrt(cr.cost(c["model"], k_dev, poses_dev[used.index(v):used.index(v) + 1], [(obj, img)]) / len(obj))
            assert abs(vout["rms"][v] - rms_v) <= 1e-9 * rms_v
        else:
            assert (vout["rvec"][v] == 0).all() and (vout["tvec"][v] == 0).all() and vout["rms"][v] == 0 and vout["reserved0"][v] == 0


@pytest.mark.parametrize("model_name,shape", ccc.CASES + [ccc.CHUNK])
def test_parity_with_the_reference(det, model_name, shape):
    c, ref = ccc.case(model_name, shape), ccc.reference(model_name, shape)
    assert ref["kept"]
    det.set_charuco_board(ccc.device_board(c["board"]))
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], cc.zero_start(c), c["n_dist"]), c["free"])
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    if shape == "chunk":
        assert list(vout["n_used"]) == [4, 31, 32, 33, 65]
    hold_to_reference(c, ref, cam, out, vout, f"{model_name} {shape}")


def test_views_that_are_skipped_and_corners_that_are_left_out(det):
    c, ref = ccc.disturbed_case(), ccc.disturbed_reference()
    assert ref["kept"]
    det.set_charuco_board(ccc.device_board(c["board"]))
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], cc.zero_start(c)), c["free"], min_markers=8)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    assert list(vout["status"]) == [_lib.CALIB_VIEW_FEW, 0, _lib.CALIB_VIEW_NO_START, 0, 0, _lib.CALIB_VIEW_FEW]
    assert list(vout["n_used"]) == [3, 72, 9, 71, 72, 7]
    hold_to_reference(c, ref, cam, out, vout, "disturbed")
    # five corners of one grid row under the default of four points a view
    c, ref = ccc.row_of_five_case(), ccc.row_of_five_reference()
    assert ref["kept"]
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], cc.zero_start(c)), c["free"])
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    assert list(vout["status"]) == [0, _lib.CALIB_VIEW_NO_START, 0] and list(vout["n_used"]) == [72, 5, 72]
    hold_to_reference(c, ref, cam, out, vout, "row of five")


def test_65_copies_of_the_3_view_case(det):
    """Past one pass of k_calib_init's lanes (195 views).  The replicated problem has the 3-view problem's stationarity equations times
    a constant: its minimiser is the 3-view reference's, and std_dev shrinks by what the formula gives (test_gpu_calibrate.py's
    test_large_calls_of_copies_of_a_16_view_case)."""
    copies = 65
    c, ref = ccc.case("plumb_bob", "3x12"), ccc.reference("plumb_bob", "3x12")
    assert ref["kept"]
    best = ref["best"]
    det.set_charuco_board(ccc.device_board(c["board"]))
    rc, cam, out, vout = calibrate(det, c["views"] * copies, c["image_size"], cam_of(c["model"], cc.zero_start(c)), c["free"])
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    assert out["n_views_used"] == 3 * copies and out["n_points"] == copies * best["n_points"]
    t = max(10.0 * ref["gap"], 1e-9)
    free = [i for i in range(16) if c["free"] >> i & 1]
    dof1 = 2 * best["n_points"] - len(best["x"])
    dofc = 2 * out["n_points"] - out["n_free"]
    k_dev = k16_of_cam(cam)
    z = np.abs(k_dev[free] - best["k16"][free]) / (2.0 * np.sqrt(2.0 * t * dof1) * best["std_dev"][free])
    sd_expected = best["std_dev"][free] * np.sqrt(dof1 / dofc)
    d_std = float(np.max(np.abs(out["std_dev"][free] - sd_expected) / sd_expected))
    d_rms = abs(out["rms"] - best["rms"]) / best["rms"]
    print(f"{3 * copies} views: status {out['status']} trials {out['n_iter']} parameters {z.max():.3e} of the bar std_dev {d_std:.3e} rms {d_rms:.3e}")
    assert z.max() <= 1.0
    assert d_std <= max(10.0 * ref["gap_std"], 1e-6) and d_rms <= max(10.0 * ref["gap_rms"], 1e-6)
    assert (vout["rvec"][:3] == vout["rvec"][3 * (copies - 1):]).all()  # (copies of a view get the same pose, to the bit)


def test_fix_aspect_the_focal_lengths_alone_and_a_given_start(det):
    c, ref = ccc.case("plumb_bob", "12x72"), ccc.reference("plumb_bob", "12x72")
    b = ccc.rboard(c["board"])
    det.set_charuco_board(ccc.device_board(c["board"]))
    # START_GIVEN from the generating camera: the reference's minimum
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(0, c["k16"]), c["free"], start=_lib.CALIB_START_GIVEN)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    hold_to_reference(c, ref, cam, out, vout, "given start")
    # FID_CALIB_FREE_FOCAL alone with one view; every other slot byte for byte
    odd = c["k16"].copy()
    odd[:2] *= (1.04, 0.97)
    odd[2:9] = (651.123456789, 349.987654321, -0.31, 0.11, 0.0007, -0.0011, -0.019)
    rc, cam, out, vout = calibrate(det, c["views"][:1], c["image_size"], cam_of(0, odd), _lib.CALIB_FREE_FOCAL, start=_lib.CALIB_START_GIVEN)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    k = k16_of_cam(cam)
    assert k[2:].tobytes() == odd[2:].tobytes() and (k[:2] != odd[:2]).all()
    assert out["n_free"] == 2 + 6 and out["n_points"] == 72 and (out["std_dev"][:2] > 0).all() and (out["std_dev"][2:] == 0).all()
    one = ccr.calibrate(b, c["views"][:1], c["image_size"], 0, odd, _lib.CALIB_FREE_FOCAL, start="given")
    cost_dev = cr.cost(0, k, poses_of(vout, [0]), one["points"])
    dof = 2 * out["n_points"] - out["n_free"]
    z = np.abs(k[:2] - one["k16"][:2]) / (2 * np.sqrt(2 * 1e-9 * dof) * one["std_dev"][:2])
    print(f"focal lengths alone, one view: cost excess {cost_dev / one['cost'] - 1:.3e} parameters {z.max():.3e} of the bar")
    assert cost_dev <= one["cost"] * (1 + 1e-9) and z.max() <= 1.0
    # fix_aspect: fx / fy stays the start's ratio
    start = c["k16"].copy()
    start[:4] *= (1.04, 1.04, 0.99, 1.01)
    rc, cam, out, _ = calibrate(det, c["views"], c["image_size"], cam_of(0, start), _lib.CALIB_FREE_PLUMB_BOB, start=_lib.CALIB_START_GIVEN, fix_aspect=1)
    assert rc == _lib.FID_OK
    k = k16_of_cam(cam)
    a = start[0] / start[1]
    assert k[0] == a * k[1] and out["std_dev"][0] == abs(a) * out["std_dev"][1] and out["n_free"] == 8 + 6 * 12
    fa = ccr.calibrate(b, c["views"], c["image_size"], 0, start, _lib.CALIB_FREE_PLUMB_BOB, fix_aspect=True, start="given", start_poses=c["poses"])
    print(f"fix_aspect: fy {k[1]} reference {fa['k16'][1]}")
    assert abs(k[1] - fa["k16"][1]) <= 2 * np.sqrt(2 * 1e-9 * (2 * out["n_points"] - out["n_free"])) * fa["std_dev"][1]


def test_refusals(det):
    c = ccc.case("plumb_bob", "3x12")
    L = det._L
    cam = cam_of(0, c["k16"])

    def refused(word, *args, **kw):
        rc, cam2, _, _ = calibrate(det, *args, **kw)
        text = L.fid_last_error(det._ctx)
        assert rc == _lib.FID_E_INVALID_ARG and text and word in text, (rc, text)
        assert bytes(cam2.c) == bytes(args[2].c)  # (views, image_size, the camera, ...)

    det.set_charuco_board(None)
    refused(b"no ChArUco board", c["views"], c["image_size"], cam, 0x1FF)
    det.set_charuco_board(ccc.device_board(c["board"]))
    bad = [(i.copy(), xy.copy()) for i, xy in c["views"]]
    bad[1][0][4] = 12  # the 5 x 4 board's corners are 0 .. 11
    refused(b"outside the board", bad, c["image_size"], cam, 0x1FF)
    bad[1][0][4] = -1
    refused(b"outside the board", bad, c["image_size"], cam, 0x1FF)
    bad = [(i.copy(), xy.copy()) for i, xy in c["views"]]
    bad[2][1][3, 1] = np.nan
    refused(b"not finite", bad, c["image_size"], cam, 0x1FF)
    one = [(c["views"][0][0][[0, 1, 4, 5]], c["views"][0][1][[0, 1, 4, 5]])]  # 8 residuals, 9 + 6 free
    assert ccr.view_status(ccc.rboard(c["board"]), one[0]) == ccr.VIEW_USED
    refused(b"residuals", one, c["image_size"], cam, 0x1FF, start=_lib.CALIB_START_GIVEN)
    refused(b"free_mask", c["views"], c["image_size"], cam, 1 << 9)  # k4 of a plumb-bob camera
    refused(b"free_mask", c["views"], c["image_size"], cam_of(2, c["k16"]), 1 << 8)  # a fifth fisheye coefficient
    assert calibrate(det, c["views"], c["image_size"], cam, 0x1FF, start=2)[0] == _lib.FID_E_INVALID_ARG
    assert calibrate(det, c["views"], c["image_size"], cam, 0x1FF, eps=float("nan"))[0] == _lib.FID_E_INVALID_ARG
    assert calibrate(det, c["views"], c["image_size"], cam, 0x1FF, min_markers=0)[0] == _lib.FID_E_INVALID_ARG
    assert calibrate(det, c["views"], (0, 720), cam, 0x1FF)[0] == _lib.FID_E_INVALID_ARG
    none = [(i[:3], xy[:3]) for i, xy in c["views"]]
    refused(b"no view can be used", none, c["image_size"], cam, 0x1FF, start=_lib.CALIB_START_GIVEN)
    refused(b"do not determine the focal lengths", none, c["image_size"], cam, 0x1FF)  # (AUTO has no view to take them from)
    packed = (np.zeros((1025, 1), _lib.CHARUCO_CORNER_DTYPE), np.zeros(1025, np.int32), 1)
    assert calibrate(det, None, c["image_size"], cam, 0x1FF, packed=packed)[0] == _lib.FID_E_INVALID_ARG
    # a batch in flight
    det.submit_batch(np.zeros((2, 480, 640), np.uint8))
    try:
        refused(b"in flight", c["views"], c["image_size"], cam, 0x1FF)
        with pytest.raises(FidError):
            det.calibrate_charuco(c["views"], c["image_size"])
    finally:
        det.collect()
    rc, _, out, _ = calibrate(det, c["views"], c["image_size"], cam, 0x1FF)
    assert rc == _lib.FID_OK and out["n_views_used"] == 3


# (model case, free mask, n_dist, coefficients of the start): between them every column of the Jacobian, test_gpu_calibrate.py's probes
PROBES = {
    "plumb_bob": ("plumb_bob", 0x01FF, 5, None),
    "equidistant": ("equidistant", 0x00FF, 4, None),
    "rational_numerator": ("rational_k124", 0x01FF, 8, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004)),
    "rational_denominator": ("rational_k124", 0x000F | 0x0E00 | 0x00C0, 8, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004)),
    "rational_prism": ("rational_k124", 0x000F | 0xF000 | 0x0030, 12, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004, 0.0009, -0.0004, -0.0007, 0.0003)),
}


@pytest.mark.parametrize("probe", list(PROBES))
def test_the_start_s_cost_and_std_dev_against_the_complex_step_jacobian(det, probe):
    """max_iter = 0 returns the start: its cost, and std_dev from the device's analytic rows over the point table at the start, held to
    the restatement's complex-step Jacobian at the same point."""
    model_name, free, n_dist, coeffs = PROBES[probe]
    c = dict(ccc.case(model_name, "12x72"), n_dist=n_dist)
    det.set_charuco_board(ccc.device_board(c["board"]))
    start = c["k16"].copy()
    start[:4] *= (1.01, 0.99, 1.005, 0.995)
    if coeffs is not None:
        start[4:4 + len(coeffs)] = coeffs
    rc, cam, out, vout = calibrate(det, c["views"], c["image_size"], cam_of(c["model"], start, c["n_dist"]), free, start=_lib.CALIB_START_GIVEN, max_iter=0)
    assert rc == _lib.FID_OK and out["status"] == _lib.CALIB_MAX_ITER and out["n_iter"] == 0
    assert bytes(cam.c) == bytes(cam_of(c["model"], start, c["n_dist"]).c)
    b = ccc.rboard(c["board"])
    pts = [ccr.view_points(b, v)[:2] for v in c["views"]]
    poses = poses_of(vout, range(len(pts)))
    prob = cr.Problem(c["model"], start, free)
    x = prob.pack(start, poses)
    sd, rms = cr.std_dev(prob, x, pts)
    cost = cr.cost(c["model"], start, poses, pts)
    fr = [i for i in range(16) if free >> i & 1]
    d = float(np.max(np.abs(out["std_dev"][fr] - sd[fr]) / sd[fr]))
    print(f"{probe}: start cost {out['cost']} vs {cost} ({out['cost'] / cost - 1:.1e}); std_dev vs complex step {d:.3e}")
    # float64 on both sides; the inverse amplifies rounding by the conditioning of J^T J: 1e-6 is the floor of the std_dev bar above
    assert abs(out["cost"] / cost - 1) <= 1e-12 and out["start_cost"] == out["cost"]
    assert abs(out["rms"] / rms - 1) <= 1e-12
    assert d <= 1e-6
    assert (out["std_dev"][[i for i in range(16) if i not in fr]] == 0).all()


def test_same_bytes_every_time(det):
    c = ccc.case("plumb_bob", "12x72")
    det.set_charuco_board(ccc.device_board(c["board"]))
    cam0 = cam_of(0, cc.zero_start(c))
    r1 = calibrate(det, c["views"], c["image_size"], cam0, c["free"])
    r2 = calibrate(det, c["views"], c["image_size"], cam0, c["free"])
    assert r1[0] == _lib.FID_OK
    same = lambda a, b: bytes(a[1].c) == bytes(b[1].c) and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert same(r1, r2)
    small = ccc.case("equidistant", "3x12")  # (another call in between, with another board and fewer views)
    det.set_charuco_board(ccc.device_board(small["board"]))
    assert calibrate(det, small["views"], small["image_size"], cam_of(2, cc.zero_start(small)), small["free"])[0] == _lib.FID_OK
    det.set_charuco_board(ccc.device_board(c["board"]))
    assert same(r1, calibrate(det, c["views"], c["image_size"], cam0, c["free"]))


def test_a_detector_that_never_calls_it_is_as_before():
    """Detection's markers and fid_last_launches with and without a board set, and calibrate_map's bytes before and after a
    calibrate_charuco on the same context."""
    import charuco_cases as chc
    from test_gpu_calibrate import calibrate as calibrate_map_raw, cam_of as map_cam_of
    d = ArucoDetector(dictionary=ccc.DICT, max_width=640, max_height=480, max_batch=8, max_markers=64)
    try:
        frames = np.ascontiguousarray(np.stack([chc.view(n).image for n in ("frontal", "tilted")]))

        def run():
            res = d.detect_markers_batch(frames)
            return b"".join(r[0].tobytes() + r[1].tobytes() for r in res), d.last_launches()

        plain = run()
        mc = cc.case("plumb_bob", "3x6")

        def map_bytes():
            d.set_map(mc["entries"])
            rc, cam, out, vout = calibrate_map_raw(d, mc["views"], mc["image_size"], map_cam_of(mc["model"], cc.zero_start(mc), mc["n_dist"]), mc["free"])
            d.set_map(None)
            assert rc == _lib.FID_OK
            return bytes(cam.c) + out.tobytes() + vout.tobytes()

        map_before = map_bytes()
        d.set_charuco_board(chc.board("5x4"))
        with_board = run()
        c = ccc.case("plumb_bob", "3x12")
        cam, out, vout = d.calibrate_charuco(c["views"], c["image_size"], max_iter=MAX_ITER, eps=EPS)
        assert out["n_views_used"] == 3
        after = run()
        assert map_bytes() == map_before
        d.set_charuco_board(None)
        assert plain == with_board == after == run()
    finally:
        d.close()


def test_end_to_end_from_rendered_views(det):
    """Eight rendered 640 x 480 views of the 5 x 4 board -> detect_markers_batch -> charuco_last without a camera -> calibrate_charuco
    (plumb-bob, fx fy cx cy k1 free, AUTO).  The answer is held to the restatement on the SAME corners.  The distance from the
    rendering camera, the rms, and the same eight frames through calibrate_map with the board as a map are printed only: nobody has
    measured them."""
    import charuco_cases as chc
    from fiducials_amd import synth
    board = chc.board("5x4")
    frames = []
    for i in range(8):
        a = 0.10 + 0.05 * i
        R, t = chc.board_pose("5x4", (a * np.cos(0.8 * i), a * np.sin(0.8 * i), 0.0), 0.30 + 0.012 * i, roll=0.4 * i,
                              shift=(0.012 * (i % 3 - 1), 0.008 * (i % 2) - 0.004))
        frames.append(synth.make_charuco_frame(chc.dictionary(), board, chc.K, R, t, seed=300 + i, width=640, height=480).image)
    det.set_charuco_board(board)
    markers = det.detect_markers_batch(np.stack(frames))
    views = det.charuco_last()
    print("end to end: markers per view", [len(ids) for _, ids in markers], "corners per view", [len(v) for v in views])
    # (a view in which detection finds few markers brings few corners or none, and is then skipped by the call like any other; the run
    # says something while most views carry most of the board)
    assert sum(len(v) >= 6 for v in views) >= 5, [len(v) for v in views]
    free = _lib.CALIB_FREE_K | 1 << 4
    cam, out, vout = det.calibrate_charuco(views, (640, 480), model=_lib.CAM_PLUMB_BOB, free=free, max_iter=MAX_ITER, eps=EPS)
    k16 = np.zeros(16)
    k16[:4] = chc.K[0, 0], chc.K[1, 1], chc.K[0, 2], chc.K[1, 2]
    c = dict(model=0, k16=k16, free=free, board="5x4", views=views, poses=None, image_size=(640, 480))
    ref = ccc.reference_of(c)
    assert ref["kept"], ref["gap"]
    hold_to_reference(c, ref, cam, out, vout, "end to end")
    k = k16_of_cam(cam)
    print(f"end to end, ChArUco corners: rms {out['rms']:.4f} px; from the rendering camera: fx {k[0] - k16[0]:+.3f} fy {k[1] - k16[1]:+.3f} "
          f"cx {k[2] - k16[2]:+.3f} cy {k[3] - k16[3]:+.3f} px, k1 {k[4]:+.5f}; std_dev fx {out['std_dev'][0]:.3f} fy {out['std_dev'][1]:.3f}")
    det.set_map(board.as_map_entries())
    try:
        mcam, mout, _ = det.calibrate_map(markers, (640, 480), model=_lib.CAM_PLUMB_BOB, free=free, max_iter=MAX_ITER, eps=EPS)
    finally:
        det.set_map(None)
    m = k16_of_cam(mcam)
    print(f"end to end, the same frames' marker corners: rms {mout['rms']:.4f} px; from the rendering camera: fx {m[0] - k16[0]:+.3f} "
          f"fy {m[1] - k16[1]:+.3f} cx {m[2] - k16[2]:+.3f} cy {m[3] - k16[3]:+.3f} px, k1 {m[4]:+.5f}; std_dev fx {mout['std_dev'][0]:.3f} "
          f"fy {mout['std_dev'][1]:.3f}")


def test_zz_print_the_largest_figures():
    print("largest over this run, in units of their bars:", WORST)
