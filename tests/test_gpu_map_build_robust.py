"""fid_build_map_robust_cam on the device against the NumPy restatement (tests/map_build_robust_restatement.py) on the planted faults
of tests/map_build_robust_cases.py.  Everything discrete (the observations' states, the outlier counts, rounds, stable, every status)
EQUALS the restatement's: the cases are kept only where no err comes near a threshold.  Cost, parameters, cov and rms are held to
the bars of tests/test_gpu_map_build.py (its hold_to_reference, imported: t from the restatement's own two-start gap on the last
solve's observations); no figure here comes from the device."""
import ctypes as C

import numpy as np
import pytest

import map_build_cases as mc
import map_build_restatement as mb
import map_build_robust_cases as rc
import map_build_robust_restatement as mbr
import test_gpu_map_build as tb
from fiducials_amd import _lib, camera
from fiducials_amd.detector import MAP_ENTRY_DTYPE, ArucoDetector
from test_map_build_robust_restatement import LARGEST_PLAIN_OFF_M, displacement, truthful

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(dictionary=6, max_width=640, max_height=480, max_batch=12, max_markers=64)
    yield d
    d.close()


def build_robust(det, c, inlier_px=rc.INLIER_PX, min_views_place=rc.MIN_VIEWS_PLACE, arrays=True, ropts_ptr=True, rout_ptr=True, **kw):
    """fid_build_map_robust_cam as it is -> (status, out, markers, views, robust_out, obs_state, obs_err, marker_outliers, view_outliers)"""
    L = det._L
    mk, n, cap = kw["packed"] if "packed" in kw else tb.pack_views(c["views"])
    opts = _lib.FidBuildOpts()
    L.fid_default_build_opts(C.byref(opts))
    opts.fiducial_len = kw.get("fiducial_len", c["fiducial_len"])
    opts.min_views = kw.get("min_views", c["min_views"])
    opts.max_iter, opts.eps, opts.sigma_px = kw.get("max_iter", tb.MAX_ITER), kw.get("eps", tb.EPS), 0.0
    lo = kw.get("len_override", c["len_override"]) or {}
    lids, lvals = np.ascontiguousarray(list(lo.keys()), dtype=np.int32), np.ascontiguousarray(list(lo.values()), dtype=np.float64)
    if len(lids):
        opts.len_ids, opts.len_values, opts.n_len = lids.ctypes.data, lvals.ctypes.data, len(lids)
    ropts = _lib.FidBuildRobustOpts(inlier_px, min_views_place, 0)
    fx = np.ascontiguousarray(kw.get("fixed", c["fixed"]), dtype=MAP_ENTRY_DTYPE).reshape(-1)
    out, rout = np.zeros(1, _lib.BUILD_OUT_DTYPE), np.zeros(1, _lib.BUILD_ROBUST_OUT_DTYPE)
    vout = np.zeros(len(n), _lib.BUILD_VIEW_DTYPE)
    cap_m = kw.get("cap_markers", max(int(n.sum()), 1))
    mout = np.zeros(max(cap_m, 1), _lib.BUILD_MARKER_DTYPE)
    n_m = C.c_int32(-5)
    state, err = np.full((len(n), cap), 255, np.uint8), np.full((len(n), cap), np.nan)
    m_outl, v_outl = np.full(max(cap_m, 1), -7, np.int32), np.full(len(n), -7, np.int32)
    cam = kw.get("cam") or tb.cam_of(c)
    rcode = L.fid_build_map_robust_cam(det._ctx, C.byref(cam.c), mk.ctypes.data, n.ctypes.data, len(n), cap, fx.ctypes.data if len(fx) else None, len(fx),
                                       C.byref(opts), C.byref(ropts) if ropts_ptr else None, out.ctypes.data if kw.get("out_ptr", True) else None, rout.ctypes.data if rout_ptr else None, mout.ctypes.data,
                                       cap_m, C.byref(n_m), vout.ctypes.data, state.ctypes.data if arrays else None, err.ctypes.data if arrays else None,
                                       m_outl.ctypes.data if arrays else None, v_outl.ctypes.data if arrays else None)
    build_robust.n_markers_out = n_m.value
    return rcode, out[0], mout[:max(n_m.value, 0)], vout, rout[0], state, err, m_outl[:max(n_m.value, 0)], v_outl


def hold_discrete(c, ref, res, label):
    rcode, out, mout, vout, rout, state, err, m_outl, v_outl = res
    o = ref["out"]
    print(f"{label}: rounds {rout['rounds']} stable {rout['stable']} n_obs {rout['n_obs']} inliers {rout['n_inliers']} outliers {rout['n_outliers']} "
          f"worst inlier {rout['worst_inlier_px']:.3f} best outlier {rout['best_outlier_px']:.3f} (restatement {o['worst_inlier_px']:.3f} {o['best_outlier_px']:.3f})")
    assert (rout["rounds"], rout["stable"], rout["n_obs"], rout["n_inliers"], rout["n_outliers"]) == (o["rounds"], o["stable"], o["n_obs"], o["n_inliers"], o["n_outliers"])
    for v, (corners, ids) in enumerate(c["views"]):
        assert list(state[v, :len(ids)]) == list(o["obs_state"][v]), (v, state[v, :len(ids)], o["obs_state"][v])
        assert (state[v, len(ids):] == _lib.OBS_NOT_KEPT).all() and (err[v, len(ids):] == -1).all()
        assert ((err[v, :len(ids)] >= 0) == (o["obs_err"][v] >= 0)).all()
    assert {int(m["id"]): int(m["status"]) for m in mout} == o["mstatus"]
    assert list(vout["status"]) == o["vstatus"]
    assert {int(m["id"]): int(k) for m, k in zip(mout, m_outl)} == o["marker_outliers"]
    assert list(v_outl) == o["view_outliers"]
    # obs_err_px: the restatement's err at the RETURNED parameters
    by_id = {int(m["id"]): m for m in mout}
    worst = 0.0
    for v, (corners, ids) in enumerate(c["views"]):
        for p, i in enumerate(ids):
            if err[v, p] < 0:
                continue
            m = by_id[int(i)]
            e = mbr.err_of(c["model"], c["k16"], (m["entry"]["R"], m["entry"]["t"]), np.concatenate([vout["rvec"][v], vout["tvec"][v]]), mb.half(m["entry"]["len"]),
                           np.asarray(corners[p], np.float64))
            if vout["status"][v] == _lib.BUILD_VIEW_USED and m["status"] in (_lib.BUILD_MARKER_FIXED, _lib.BUILD_MARKER_SOLVED):
                worst = max(worst, abs(e - err[v, p]))
    print(f"{label}: obs_err_px against the restatement at the returned parameters: {worst:.2e} px")
    assert worst <= 1e-9
    # the two figures of the record are the arrays' own
    n_of = [len(ids) for _, ids in c["views"]]
    inl = [err[v, p] for v in range(len(n_of)) for p in range(n_of[v]) if state[v, p] == _lib.OBS_INLIER]
    outl = [err[v, p] for v in range(len(n_of)) for p in range(n_of[v]) if state[v, p] == _lib.OBS_OUTLIER and err[v, p] >= 0]
    assert rout["worst_inlier_px"] == (max(inl) if inl else -1.0) and rout["best_outlier_px"] == (min(outl) if outl else -1.0)


def same_branch(ref, vout):
    """A rotation by nearly a half turn has two vectors, r and r (1 - 2 pi / |r|), and a camera that looks straight at a wall is
    nearly one: where a view's vector and the reference's are the two branches of one rotation, the device's is written on the
    reference's branch before the parameters are compared (the views' vectors are compared as they are returned, the markers' go
    through their matrices).  Nothing else of the record is touched."""
    vout = vout.copy()
    for v in ref["best"]["used"]:
        r, want = vout["rvec"][v].copy(), ref["best"]["vposes"][v][:3]
        other = r * (1.0 - 2.0 * np.pi / np.linalg.norm(r))
        if np.linalg.norm(other - want) < np.linalg.norm(r - want):
            print(f"view {v}: |rvec| {np.linalg.norm(r):.6f}, the reference's {np.linalg.norm(want):.6f}: the other branch of the same rotation")
            vout["rvec"][v] = other
    return vout


@pytest.mark.parametrize("name", rc.CASES + (rc.WALL,))
def test_planted_faults_against_the_restatement(det, name):
    c, ref = rc.case(name), rc.reference(name)
    assert ref["kept"], (ref["gap"], mbr.band_clear(ref["out"]))
    res = build_robust(det, c)
    assert res[0] == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    hold_discrete(c, ref, res, name)
    tb.hold_to_reference(ref, res[1], res[2], same_branch(ref, res[3]), name)


@pytest.mark.parametrize("name", ["moved", "swap_equidistant", "many_views", rc.WALL])
def test_the_start_s_errors_agree_with_the_restatement_far_inside_the_clearance(det, name):
    """The first set is decided under the start's poses, and the cases are kept where every err there clears inlier_px by more than 1
    % (map_build_robust_restatement.band_clear).  That clearance is enough only if the device's start and NumPy's agree far better:
    with max_iter 0 the call returns the start (its one round moves nothing), so obs_err_px is err under the device's start.  Held
    to a tenth of the clearance."""
    c, ref = rc.case(name), rc.reference(name)
    res = build_robust(det, c, max_iter=0)
    assert res[0] == _lib.FID_OK and res[1]["n_iter"] == 0
    thr0, e0 = ref["out"]["first_set"]
    worst = max(abs(res[6][v, p] - e) for (v, p), e in e0.items())
    assert all(res[6][v, p] >= 0 for v, p in e0) and int((res[6] >= 0).sum()) == len(e0)
    print(f"{name}: err under the start, device against NumPy: {worst:.3e} px over {len(e0)} observations (clearance {0.01 * thr0} px)")
    assert worst <= 0.1 * 0.01 * thr0


def test_nothing_planted_is_the_plain_call_within_the_bars(det):
    c, ref = rc.case("clean"), mc.reference("views16")
    rob, plain = build_robust(det, c), tb.build(det, c)
    assert rob[0] == plain[0] == _lib.FID_OK
    assert rob[4]["rounds"] == 1 and rob[4]["stable"] == 1 and rob[4]["n_outliers"] == 0 and (rob[7] == 0).all() and (rob[8] == 0).all()
    t = max(10.0 * ref["gap"], 1e-9)
    best = ref["best"]
    xr, xp = tb.device_x(ref, rob[2], rob[3]), tb.device_x(ref, plain[2], plain[3])
    z = np.abs(xr - xp) / (2.0 * np.sqrt(2.0 * t * best["dof"]) * best["std"])
    cr, cp = (float(best["problem"].res(x) @ best["problem"].res(x)) for x in (xr, xp))
    print(f"clean: robust against plain: parameters {z.max():.3e} of the bar, cost {cr / cp - 1:.3e} (bar {t:.1e})")
    assert z.max() <= 1.0 and cr <= cp * (1 + t) and cp <= cr * (1 + t)
    assert rob[1]["n_points"] == plain[1]["n_points"] and list(rob[3]["status"]) == list(plain[3]["status"])


def test_the_attacked_start_the_plain_call_is_off_the_robust_one_is_not(det):
    c = rc.case("largest")
    plain = tb.build(det, c)
    rob = build_robust(det, c)
    assert plain[0] == rob[0] == _lib.FID_OK
    truth = {i: p[3:] for i, p in truthful(c)["best"]["mposes"].items()}
    d_plain = displacement({int(m["id"]): m["entry"]["t"] for m in plain[2] if m["status"] == _lib.BUILD_MARKER_SOLVED}, truth)
    d_rob = displacement({int(m["id"]): m["entry"]["t"] for m in rob[2] if m["status"] == _lib.BUILD_MARKER_SOLVED}, truth)
    print(f"largest: worst marker off by {d_plain * 1e3:.2f} mm in the plain call, {d_rob * 1e3:.3f} mm in the robust one (bound {LARGEST_PLAIN_OFF_M * 1e3} mm)")
    assert d_plain > LARGEST_PLAIN_OFF_M
    tb.hold_to_reference(rc.reference("largest"), rob[1], rob[2], rob[3], "largest")


def test_same_bytes_and_null_arrays_and_python(det):
    c = rc.case("moved")
    a, b = build_robust(det, c), build_robust(det, c)
    assert a[0] == _lib.FID_OK
    for p, q in zip(a[1:], b[1:]):
        assert p.tobytes() == q.tobytes()
    n = build_robust(det, c, arrays=False)
    assert n[0] == _lib.FID_OK
    for p, q in zip(a[1:5], n[1:5]):
        assert p.tobytes() == q.tobytes()
    py = det.build_map_robust(c["views"], tb.cam_of(c), c["fiducial_len"], c["fixed"], rc.INLIER_PX, rc.MIN_VIEWS_PLACE, min_views=c["min_views"], max_iter=tb.MAX_ITER,
                              eps=tb.EPS)
    assert py[1].tobytes() == a[1].tobytes() and py[2].tobytes() == a[2].tobytes() and py[3].tobytes() == a[3].tobytes() and py[4].tobytes() == a[4].tobytes()
    for v, (_, ids) in enumerate(c["views"]):
        assert py[5][v].tobytes() == a[5][v, :len(ids)].tobytes() and py[6][v].tobytes() == a[6][v, :len(ids)].tobytes()
    assert py[7].tobytes() == a[7].tobytes() and py[8].tobytes() == a[8].tobytes()


def test_refusals(det):
    c = rc.case("swap_plumb_bob")
    inv = _lib.FID_E_INVALID_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert build_robust(det, c, inlier_px=bad)[0] == inv
    assert b"inlier_px" in det._L.fid_last_error(det._ctx)
    assert build_robust(det, c, min_views_place=0)[0] == inv
    assert build_robust(det, c, ropts_ptr=False)[0] == inv and build_robust(det, c, rout_ptr=False)[0] == inv
    # every refusal of the plain call (tests/test_gpu_map_build.py::test_refusals, in its order)
    err_text = lambda: det._L.fid_last_error(det._ctx)
    assert build_robust(det, c, out_ptr=False)[0] == inv and b"NULL" in err_text() and build_robust.n_markers_out == 0
    assert build_robust(det, c, packed=(np.zeros((4097, 1), tb.MARKER_DT), np.zeros(4097, np.int32), 1))[0] == inv
    assert build_robust(det, c, packed=(np.zeros((0, 1), tb.MARKER_DT), np.zeros(0, np.int32), 1))[0] == inv
    mk, n, cap = tb.pack_views(c["views"])
    assert build_robust(det, c, packed=(mk, n, 0))[0] == inv
    assert build_robust(det, c, len_override={3: -1.0})[0] == inv
    rcap = build_robust(det, c, cap_markers=3)
    assert rcap[0] == _lib.FID_E_CAPACITY and b"6" in err_text() and build_robust.n_markers_out == 6  # (the count is reported)
    # the robust call's own checks come first, but its refusals leave the count at 0 too
    assert build_robust(det, c, inlier_px=-1.0, cap_markers=3)[0] == inv and build_robust.n_markers_out == 0
    assert build_robust(det, c, fixed=np.zeros(0, MAP_ENTRY_DTYPE))[0] == inv
    assert build_robust(det, c, fixed=np.concatenate([c["fixed"], c["fixed"]]))[0] == inv and b"twice" in det._L.fid_last_error(det._ctx)
    assert build_robust(det, c, fiducial_len=0.0)[0] == inv
    assert build_robust(det, c, min_views=0)[0] == inv
    assert build_robust(det, c, eps=float("nan"))[0] == inv
    unusable = tb.cam_of(c)
    unusable.c.model = 7
    assert build_robust(det, c, cam=unusable)[0] == inv
    bad = dict(c, views=[(v[0].copy(), v[1]) for v in c["views"]])
    bad["views"][1][0][2, 1, 0] = np.inf
    assert build_robust(det, bad)[0] == inv and b"not finite" in det._L.fid_last_error(det._ctx)
    assert build_robust(det, dict(c, views=[(v[0], v[1] + 900) for v in c["views"]]))[0] == inv  # no view holds a fixed fiducial
    many = mc.case(mc.TOO_MANY)
    assert build_robust(det, dict(many, planted=frozenset()))[0] == _lib.FID_E_UNSUPPORTED
    assert build_robust(det, c)[0] == _lib.FID_OK


def test_the_plain_call_and_the_context_are_untouched(det):
    from aruco_map_cases import K as K_MAP, scene, scene_map
    frames = np.stack([scene("3x2", p).image for p in range(3)])
    det.set_map(scene_map("3x2"))
    mcam = camera.Camera(0, K_MAP, np.zeros(5))
    det_before = det.detect_markers_batch(frames)
    pose_before = det.map_pose_last(camera=mcam).tobytes()
    single_before = [(p.rvecs.tobytes(), p.tvecs.tobytes()) for p in det.pose_last(0.08, camera=mcam)]
    c = mc.case("size11")
    p1 = tb.build(det, c)
    assert build_robust(det, rc.case("swap"))[0] == _lib.FID_OK
    p2 = tb.build(det, c)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(p1[1:], p2[1:]))
    assert det.map_pose_last(camera=mcam).tobytes() == pose_before
    assert [(p.rvecs.tobytes(), p.tvecs.tobytes()) for p in det.pose_last(0.08, camera=mcam)] == single_before
    for (ca, ia), (cb, ib) in zip(det_before, det.detect_markers_batch(frames)):
        assert ca.tobytes() == cb.tobytes() and ia.tobytes() == ib.tobytes()
    det.submit_batch(frames)
    assert build_robust(det, rc.case("swap"))[0] == _lib.FID_E_INVALID_ARG  # a batch in flight
    det.collect()
    det.set_map(None)
