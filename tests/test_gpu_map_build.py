"""fid_build_map_cam on the device against the NumPy restatement (tests/map_build_restatement.py) on the cases of
tests/map_build_cases.py.  Frames are 640 x 480.

THE BARS are the calibration's (tests/test_gpu_calibrate.py), none chosen from what the device gives.  With t = max(10 x the
reference's own two-start cost gap of the case, 1e-9):
  cost        the device's answer, evaluated by the restatement's residual function, costs at most the reference minimum x (1 + t)
  parameters  every parameter (the six of every solved marker, the six of every used view) within 2 sqrt(2 t dof) reference standard
              deviations
  cov, rms    cov's diagonals and rms relative, at most max(10 x the reference's two-start gap in them, 1e-6)

MEASURED ON THE MI355X, the largest over this file in units of the bars: see test_zz_print_the_largest_figures' output, copied into
DESIGN.md's section "building the map"."""
import ctypes as C

import numpy as np
import pytest

import map_build_cases as mc
import map_build_restatement as mb
from fiducials_amd import _lib, camera
from fiducials_amd.detector import MAP_ENTRY_DTYPE, ArucoDetector

pytestmark = pytest.mark.gpu

MARKER_DT = np.dtype([("id", "<i4"), ("corners", "<f4", (8,))])
N_DIST = {0: 5, 1: 8, 2: 4}
MAX_ITER = 3000
EPS = 1e-15  # the reference's own standstill (map_build_restatement.lm's rel_step), not the header's default
WORST = {"cost": 0.0, "param": 0.0, "cov": 0.0, "rms": 0.0}


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(dictionary=6, max_width=640, max_height=480, max_batch=12, max_markers=64)
    yield d
    d.close()


def cam_of(c):
    k = c["k16"]
    return camera.Camera(c["model"], [[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]], k[4:4 + N_DIST[c["model"]]])


def pack_views(views):
    views = [(np.asarray(cn, np.float32).reshape(-1, 8), np.asarray(i, np.int32).reshape(-1)) for cn, i in views]
    cap = max([len(i) for _, i in views] + [1])
    mk = np.zeros((len(views), cap), MARKER_DT)
    n = np.zeros(len(views), np.int32)
    for v, (cn, i) in enumerate(views):
        n[v] = len(i)
        mk["id"][v, :len(i)] = i
        mk["corners"][v, :len(i)] = cn
    return mk, n, cap


def build(det, c, views=None, fixed="case", max_iter=MAX_ITER, eps=EPS, sigma_px=0.0, min_views=None, fiducial_len=None, cam=None, packed=None,
          cap_markers=None, len_override="case", out_ptr=True):
    """fid_build_map_cam as it is -> (status, out record, markers array, views array)"""
    L = det._L
    mk, n, cap = packed if packed is not None else pack_views(c["views"] if views is None else views)
    opts = _lib.FidBuildOpts()
    L.fid_default_build_opts(C.byref(opts))
    opts.fiducial_len = c["fiducial_len"] if fiducial_len is None else fiducial_len
    opts.min_views = c["min_views"] if min_views is None else min_views
    opts.max_iter, opts.eps, opts.sigma_px = max_iter, eps, sigma_px
    lo = c["len_override"] if len_override == "case" else len_override
    lids = np.ascontiguousarray(list((lo or {}).keys()), dtype=np.int32)
    lvals = np.ascontiguousarray(list((lo or {}).values()), dtype=np.float64)
    if len(lids):
        opts.len_ids, opts.len_values, opts.n_len = lids.ctypes.data, lvals.ctypes.data, len(lids)
    fx = np.ascontiguousarray(c["fixed"] if isinstance(fixed, str) else fixed, dtype=MAP_ENTRY_DTYPE).reshape(-1)
    out = np.zeros(1, _lib.BUILD_OUT_DTYPE)
    vout = np.zeros(len(n), _lib.BUILD_VIEW_DTYPE)
    cap_m = max(int(n.sum()), 1) if cap_markers is None else cap_markers
    mout = np.zeros(max(cap_m, 1), _lib.BUILD_MARKER_DTYPE)
    n_m = C.c_int32(0)
    cam = cam_of(c) if cam is None else cam
    rc = L.fid_build_map_cam(det._ctx, C.byref(cam.c), mk.ctypes.data, n.ctypes.data, len(n), cap, fx.ctypes.data if len(fx) else None, len(fx), C.byref(opts),
                             out.ctypes.data if out_ptr else None, mout.ctypes.data, cap_m, C.byref(n_m), vout.ctypes.data)
    return rc, out[0], mout[:n_m.value], vout


def device_x(ref, mout, vout):
    """The device's answer as the restatement's parameter vector."""
    best = ref["best"]
    by_id = {int(m["id"]): m for m in mout}
    mposes = {}
    for i in best["mposes"]:
        m = by_id[i]
        assert m["status"] == _lib.BUILD_MARKER_SOLVED, (i, m["status"])
        mposes[best["slot"][i]] = np.concatenate([mb.rotation_vector(m["entry"]["R"]), m["entry"]["t"]])
    return best["problem"].pack(mposes, [np.concatenate([vout["rvec"][v], vout["tvec"][v]]) for v in best["used"]])


def hold_to_reference(ref, out, mout, vout, label):
    """The bars of the module docstring, the figures printed first."""
    best = ref["best"]
    prob = best["problem"]
    used = [v for v in range(len(vout)) if vout["status"][v] == _lib.BUILD_VIEW_USED]
    assert used == best["used"], (used, best["used"])
    solved = sorted(int(m["id"]) for m in mout if m["status"] == _lib.BUILD_MARKER_SOLVED)
    assert solved == sorted(best["mposes"]), (solved, sorted(best["mposes"]))
    x_dev = device_x(ref, mout, vout)
    r = prob.res(x_dev)
    cost_dev = float(r @ r)
    t = max(10.0 * ref["gap"], 1e-9)
    dof = best["dof"]
    excess = cost_dev / best["cost"] - 1.0
    z = np.abs(x_dev - best["x"]) / (2.0 * np.sqrt(2.0 * t * dof) * best["std"])
    bar_cov, bar_rms = max(10.0 * ref["gap_cov"], 1e-6), max(10.0 * ref["gap_rms"], 1e-6)
    by_id = {int(m["id"]): m for m in mout}
    d_cov = max([float(np.max(np.abs(np.diag(by_id[i]["cov"]) - np.diag(best["cov"][i])) / np.diag(best["cov"][i]))) for i in best["cov"]] + [0.0])
    d_rms = abs(out["rms"] - best["rms"]) / best["rms"]
    print(f"{label}: status {out['status']} trials {out['n_iter']} n {6 * len(solved)} cost excess {excess:.3e} (bar {t:.1e}) parameters {z.max():.3e} of the bar "
          f"cov {d_cov:.3e} (bar {bar_cov:.1e}) rms {d_rms:.3e} (bar {bar_rms:.1e}) reported cost vs restatement {out['cost'] / cost_dev - 1:.1e}")
    for key, val in (("cost", excess / t), ("param", z.max()), ("cov", d_cov / bar_cov), ("rms", d_rms / bar_rms)):
        WORST[key] = max(WORST[key], float(val))
    assert out["n_points"] == best["n_points"] and out["n_views_used"] == len(used) and out["n_free"] == best["n_free"]
    assert cost_dev <= best["cost"] * (1.0 + t)
    assert out["cost"] <= out["start_cost"]
    assert z.max() <= 1.0
    assert d_cov <= bar_cov
    assert d_rms <= bar_rms
    for i in best["cov"]:  # symmetric, and the per-marker and per-view rms are the restatement's
        assert np.allclose(by_id[i]["cov"], by_id[i]["cov"].T, rtol=1e-9, atol=0)
        assert abs(by_id[i]["rms"] - best["mrms"][i]) <= 1e-6 * best["mrms"][i]
    for v in used:
        assert abs(vout["rms"][v] - best["vrms"][v]) <= 1e-6 * best["vrms"][v]


def run_case(det, name):
    c, ref = mc.case(name), mc.reference(name)
    assert ref["kept"], ref["gap"]
    rc, out, mout, vout = build(det, c)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    hold_to_reference(ref, out, mout, vout, name)
    return c, ref, out, mout, vout


def test_chain_of_three_with_min_views_1(det):
    c, ref, out, mout, vout = run_case(det, "chain3_min1")
    assert list(mout["id"]) == [0, 1, 2] and list(mout["status"]) == [_lib.BUILD_MARKER_FIXED, _lib.BUILD_MARKER_SOLVED, _lib.BUILD_MARKER_SOLVED]
    assert list(mout["n_views"]) == [2, 3, 1] and out["n_markers"] == 3 and out["n_fixed"] == 1
    assert mout["entry"][0].tobytes() == c["fixed"][0].tobytes() and (mout["cov"][0] == 0).all()
    # links: A - B, B - A and C, C - B
    assert [int(m["links"][0]) for m in mout] == [0b011, 0b111, 0b110]


def test_chain_of_three_with_min_views_2(det):
    c, ref, out, mout, vout = run_case(det, "chain3_min2")
    assert list(mout["status"]) == [_lib.BUILD_MARKER_FIXED, _lib.BUILD_MARKER_SOLVED, _lib.BUILD_MARKER_FEW_VIEWS]
    assert list(vout["status"]) == [0, 0, 0] and list(vout["n_used"]) == [2, 1, 2]  # view 1 from B alone
    assert (mout["cov"][2] == 0).all() and mout["slot"][2] == -1 and mout["rms"][2] == 0


def test_two_components(det):
    c, ref, out, mout, vout = run_case(det, "two_components")
    st = {int(m["id"]): int(m["status"]) for m in mout}
    assert st[10] == st[11] == _lib.BUILD_MARKER_UNREACHED
    assert list(vout["status"]) == [0, 0, 0, 0, _lib.BUILD_VIEW_UNREACHED, _lib.BUILD_VIEW_UNREACHED]
    assert (vout["rvec"][4:] == 0).all() and (vout["n_used"][4:] == 0).all()


@pytest.mark.parametrize("name", ["size10", "size11", "size21", "size22"])
def test_reduced_system_sizes_across_the_tile_edges(det, name):
    c, ref, out, mout, vout = run_case(det, name)
    assert out["n_markers"] - out["n_fixed"] == int(name[4:])


def test_128_markers_in_the_solve(det):
    c, ref, out, mout, vout = run_case(det, mc.LARGE)
    assert out["n_markers"] == 128 and out["n_fixed"] == 1


def test_129_markers_are_refused(det):
    c = mc.case(mc.TOO_MANY)
    rc, out, mout, vout = build(det, c)
    assert rc == _lib.FID_E_UNSUPPORTED
    assert b"129" in det._L.fid_last_error(det._ctx)


def test_views_of_64_and_65_listed_markers(det):
    c, ref, out, mout, vout = run_case(det, "lists")
    assert list(vout["n_over"]) == [0, 1, 16, 0] and list(vout["n_used"]) == [64, 64, 64, 64]
    assert len(mout) == 64 and out["n_fixed"] == 4


def test_an_id_twice_a_length_override_and_two_fixed_entries(det):
    c, ref, out, mout, vout = run_case(det, "mixed")
    assert out["n_fixed"] == 2 and vout["n_used"][2] == len(c["views"][2][1]) - 2  # both records of id 3 are out of view 2
    by_id = {int(m["id"]): m for m in mout}
    assert by_id[7]["entry"]["len"] == 0.09375 and by_id[6]["entry"]["len"] == c["fiducial_len"]
    assert by_id[3]["n_views"] == sum(1 for _, i in c["views"] if (np.asarray(i) == 3).sum() == 1)
    # without the override the marker's own side is wrong and the minimum is visibly worse
    rc, out2, _, _ = build(det, c, len_override=None)
    assert rc == _lib.FID_OK and out2["cost"] > 2 * out["cost"]


@pytest.mark.parametrize("cam", ["plumb_bob", "rational", "equidistant"])
def test_each_camera_model(det, cam):
    run_case(det, "model_" + cam)


def test_a_plumb_bob_camera_is_the_rational_one_with_zeros_to_the_byte(det):
    """k_build_blocks and k_build_eval run the rational instantiation for a plumb-bob camera (fid_map_build.hip): the same call with
    the camera handed in as FID_CAM_RATIONAL, k4 k5 k6 zero, returns the same bytes, start included."""
    c = mc.case("model_plumb_bob")
    k = c["k16"]
    rational = camera.Camera(_lib.CAM_RATIONAL, [[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]], list(k[4:9]) + [0.0, 0.0, 0.0])
    a, b = build(det, c), build(det, c, cam=rational)
    assert a[0] == b[0] == _lib.FID_OK
    assert a[1]["n_iter"] > 5
    for p, q in zip(a[1:], b[1:]):
        assert p.tobytes() == q.tobytes()


def test_views_and_markers_without_a_start_are_reported_and_left_out(det):
    """The fisheye model cannot pose a marker with a corner at 89 degrees or more off the axis.  Two views that hold the fixed marker
    there are reached but get no start (FID_BUILD_VIEW_NO_START); a marker that only they hold is never placed
    (FID_BUILD_MARKER_NO_START), its slot goes to the next id, and the rest of the call is the call without the two views."""
    c = mc.case("model_equidistant")
    twice = lambda views: [(cn, i * 2) for cn, i in views]  # ids 0 2 4 ..: room for id 3 in the middle of the slots
    fixed = c["fixed"].copy()
    fixed["id"] *= 2
    plain = build(det, c, views=twice(c["views"]), fixed=fixed)
    assert plain[0] == _lib.FID_OK
    cn0, i0 = c["views"][0]
    at = int(np.nonzero(i0 == 0)[0][0])
    far = [(np.concatenate([cn0[at:at + 1] + 2000.0, cn0[at + 1:at + 2] + d]), np.array([0, 3], np.int32)) for d in (0.0, 1.0)]
    rc, out, mout, vout = build(det, c, views=twice(c["views"]) + far, fixed=fixed)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    n = len(c["views"])
    assert list(vout["status"][n:]) == [_lib.BUILD_VIEW_NO_START] * 2 and (vout["rvec"][n:] == 0).all() and (vout["n_used"][n:] == 0).all()
    by_id = {int(m["id"]): m for m in mout}
    assert by_id[3]["status"] == _lib.BUILD_MARKER_NO_START and by_id[3]["slot"] == -1 and by_id[3]["n_views"] == 2 and (by_id[3]["cov"] == 0).all()
    assert [int(m["slot"]) for m in mout if m["id"] != 3] == list(range(len(mout) - 1))
    assert out.tobytes() == plain[1].tobytes() and vout[:n].tobytes() == plain[3].tobytes()
    for m in plain[2]:
        q = by_id[int(m["id"])].copy()
        if m["id"] == 0:
            q["n_views"] -= 2  # (the fixed marker is kept by the two views as well)
        assert q.tobytes() == m.tobytes()


def test_two_walls(det):
    run_case(det, "corner")


@pytest.mark.parametrize("copies", [1, 4, 16])
def test_copies_of_a_16_view_case(det, copies):
    """The replicated problem: with every view `copies` times the stationarity equations are the 16-view problem's times a constant,
    so the minimiser is the 16-view reference's.  J^T J's complement over the markers grows by `copies` and the cost by `copies`; the
    degrees of freedom are 2 N copies - (n_m + 6 V copies) with n_m the markers' parameters.  So cov shrinks by
    (dof_1 / dof_c) -- cost_c / dof_c x 1 / copies against cost_1 / dof_1."""
    c, ref = mc.case("views16"), mc.reference("views16")
    assert ref["kept"]
    best = ref["best"]
    rc, out, mout, vout = build(det, c, views=c["views"] * copies)
    assert rc == _lib.FID_OK, det._L.fid_last_error(det._ctx)
    assert out["n_views_used"] == 16 * copies and out["n_points"] == copies * best["n_points"]
    t = max(10.0 * ref["gap"], 1e-9)
    dof1, dofc = best["dof"], 2 * int(out["n_points"]) - int(out["n_free"])
    x_dev = device_x(ref, mout, vout[:16])
    z = np.abs(x_dev - best["x"]) / (2.0 * np.sqrt(2.0 * t * dof1) * best["std"])
    by_id = {int(m["id"]): m for m in mout}
    d_cov = max(float(np.max(np.abs(np.diag(by_id[i]["cov"]) - np.diag(best["cov"][i]) * dof1 / dofc) / (np.diag(best["cov"][i]) * dof1 / dofc))) for i in best["cov"])
    d_rms = abs(out["rms"] - best["rms"]) / best["rms"]
    print(f"{16 * copies} views: status {out['status']} trials {out['n_iter']} parameters {z.max():.3e} of the bar cov {d_cov:.3e} rms {d_rms:.3e}")
    assert z.max() <= 1.0
    assert d_cov <= max(10.0 * ref["gap_cov"], 1e-6) and d_rms <= max(10.0 * ref["gap_rms"], 1e-6)
    assert vout["rvec"][:16].tobytes() == vout["rvec"][16 * (copies - 1):].tobytes()  # (copies of a view get the same pose, to the bit)
    assert vout["tvec"][:16].tobytes() == vout["tvec"][16 * (copies - 1):].tobytes()


@pytest.mark.parametrize("name", ["corner", "model_rational", "model_equidistant", "size11"])
def test_the_start_s_cost_and_cov_against_the_complex_step_jacobian(det, name):
    """max_iter = 0 returns the start: its cost, and cov from the device's analytic Jacobian (every column of marker and view) at the
    start, held to the restatement's complex-step Jacobian at the same point.  sigma_px scales cov as stated."""
    c, ref = mc.case(name), mc.reference(name)
    rc, out, mout, vout = build(det, c, max_iter=0)
    assert rc == _lib.FID_OK and out["status"] == _lib.BUILD_MAX_ITER and out["n_iter"] == 0
    prob = ref["best"]["problem"]
    x = device_x(ref, mout, vout)
    cov, std, cost, dof = mb.covariance(prob, x)
    by_id = {int(m["id"]): m for m in mout}
    inv = {s: i for i, s in ref["best"]["slot"].items()}
    d = max(float(np.max(np.abs(by_id[inv[s]]["cov"] - cov[s]) / np.sqrt(np.outer(np.diag(cov[s]), np.diag(cov[s]))))) for s in cov)
    print(f"{name}: start cost {out['cost']} vs {cost} ({out['cost'] / cost - 1:.1e}); cov vs complex step {d:.3e}")
    # float64 on both sides; the marker's rotation vector goes through the returned matrix and back, and the inverse amplifies rounding by
    # the conditioning of J^T J: 1e-6 is the floor of the cov bar above
    assert abs(out["cost"] / cost - 1) <= 1e-9 and out["start_cost"] == out["cost"]
    assert d <= 1e-6
    rc, out2, mout2, _ = build(det, c, max_iter=0, sigma_px=0.5)
    assert rc == _lib.FID_OK
    f = 0.25 / (cost / dof)
    for m, m2 in zip(mout, mout2):
        if m["status"] == _lib.BUILD_MARKER_SOLVED:
            assert np.allclose(m2["cov"], m["cov"] * f, rtol=1e-9, atol=0)


def test_same_bytes_every_time_and_the_other_calls_untouched(det):
    from aruco_map_cases import K as K_MAP, scene, scene_map
    import calib_cases as cc
    frames = np.stack([scene("3x2", p).image for p in range(3)])
    det.set_map(scene_map("3x2"))
    mcam = camera.Camera(0, K_MAP, np.zeros(5))
    det_before = det.detect_markers_batch(frames)
    pose_before = det.map_pose_last(camera=mcam).tobytes()
    single_before = [(p.rvecs.tobytes(), p.tvecs.tobytes()) for p in det.pose_last(0.08, camera=mcam)]
    cal = cc.case("plumb_bob", "3x6")
    c = mc.case("size11")
    r1 = build(det, c)
    r2 = build(det, c)
    assert r1[0] == _lib.FID_OK
    same = lambda a, b: all(p.tobytes() == q.tobytes() for p, q in zip(a[1:], b[1:]))
    assert same(r1, r2)
    det_after = det.detect_markers_batch(frames)
    assert det.map_pose_last(camera=mcam).tobytes() == pose_before  # (the context's map is untouched)
    assert [(p.rvecs.tobytes(), p.tvecs.tobytes()) for p in det.pose_last(0.08, camera=mcam)] == single_before
    for (ca, ia), (cb, ib) in zip(det_before, det_after):
        assert ca.tobytes() == cb.tobytes() and ia.tobytes() == ib.tobytes()
    # a calibration before and after
    det.set_map(cal["entries"])
    k1 = det.calibrate_map(cal["views"], cal["image_size"], max_iter=50)
    r3 = build(det, c)
    k2 = det.calibrate_map(cal["views"], cal["image_size"], max_iter=50)
    assert same(r1, r3)
    assert bytes(k1[0].c) == bytes(k2[0].c) and k1[1].tobytes() == k2[1].tobytes() and k1[2].tobytes() == k2[2].tobytes()
    # a batch in flight is refused
    det.submit_batch(frames)
    assert build(det, c)[0] == _lib.FID_E_INVALID_ARG
    det.collect()
    assert same(r1, build(det, c))


def test_refusals(det):
    c = mc.case("model_plumb_bob")
    L = det._L
    err = lambda: L.fid_last_error(det._ctx)
    inv = _lib.FID_E_INVALID_ARG
    assert build(det, c, fixed=np.zeros(0, MAP_ENTRY_DTYPE))[0] == inv  # no fixed entry (a NULL pointer)
    assert build(det, c, out_ptr=False)[0] == inv and b"NULL" in err()
    assert build(det, c, fixed=np.concatenate([c["fixed"], c["fixed"]]))[0] == inv and b"twice" in err()
    assert build(det, c, packed=(np.zeros((4097, 1), MARKER_DT), np.zeros(4097, np.int32), 1))[0] == inv
    assert build(det, c, packed=(np.zeros((0, 1), MARKER_DT), np.zeros(0, np.int32), 1))[0] == inv
    mk, n, cap = pack_views(c["views"])
    assert build(det, c, packed=(mk, n, 0))[0] == inv
    bad = [(v[0].copy(), v[1]) for v in c["views"]]
    bad[1][0][2, 1, 0] = np.inf
    assert build(det, c, views=bad)[0] == inv and b"not finite" in err()
    assert build(det, c, fiducial_len=0.0)[0] == inv
    assert build(det, c, len_override={3: -1.0})[0] == inv
    assert build(det, c, min_views=0)[0] == inv
    assert build(det, c, eps=float("nan"))[0] == inv
    unusable = cam_of(c)
    unusable.c.model = 7
    assert build(det, c, cam=unusable)[0] == inv
    rc, _, mout, _ = build(det, c, cap_markers=3)
    assert rc == _lib.FID_E_CAPACITY and b"6" in err()
    lost = [(v[0], v[1] + 900) for v in c["views"]]
    assert build(det, c, views=lost)[0] == inv  # no view holds a fixed fiducial
    assert build(det, c)[0] == _lib.FID_OK


def test_end_to_end_from_rendered_views(det):
    """Ten rendered 640 x 480 views of a two-wall scene of 8 markers -> detect_markers_batch -> build_map with marker 20 fixed at its
    true pose.  The answer is held to the restatement on the SAME detected corners; then set_map(entries) and map_pose_last on a
    further rendered frame.  The distances from the rendering poses are printed only (nobody has measured the corner bias)."""
    from aruco_map_cases import K as K_MAP, corner_of_two_walls, look_at
    from fiducials_amd import synth
    from fiducials_amd.dictionary import get_predefined_dictionary
    scene = corner_of_two_walls(4, 4, first_id=20)
    spec = [(float(e["len"]), e["R"], e["t"]) for e in scene]
    rng = np.random.default_rng(31)
    frames, poses = [], []
    for i in range(11):
        pos = np.array([rng.uniform(0.55, 0.8), rng.uniform(-0.05, 0.3), rng.uniform(0.55, 0.8)])
        R, t = look_at(pos, np.array([0.15, 0.1, 0.15]))
        frames.append(synth.make_aruco_board_frame(get_predefined_dictionary(6), scene["id"], spec, K_MAP, R, t, 300 + i, 640, 480).image)
        poses.append((R, t))
    views = det.detect_markers_batch(np.stack(frames[:10]))
    print("end to end: markers per view", [len(i) for _, i in views])
    assert all(len(i) >= 2 for _, i in views)
    cam = camera.Camera(0, K_MAP, np.zeros(5))
    entries, out, mout, vout = det.build_map(views, cam, 0.125, scene[:1], max_iter=MAX_ITER, eps=EPS)
    k16 = np.zeros(16)
    k16[:4] = K_MAP[0, 0], K_MAP[1, 1], K_MAP[0, 2], K_MAP[1, 2]
    c = dict(model=0, k16=k16, views=views, fixed=scene[:1], fiducial_len=0.125, len_override=None, min_views=2,
             true_markers=mc._true_markers(scene), poses=[np.concatenate([mb.rotation_vector(R), t]) for R, t in poses[:10]])
    ref = mc.reference_of(c)
    assert ref["kept"], ref["gap"]
    hold_to_reference(ref, out, mout, vout, "end to end")
    dist = [float(np.linalg.norm(e["t"] - scene[scene["id"] == e["id"]][0]["t"])) for e in entries]
    print(f"end to end: rms {out['rms']:.4f} px; built markers from the scene: at most {max(dist) * 1000:.2f} mm")
    det.set_map(entries)
    det.detect_markers_batch(np.stack(frames[10:]))
    p = det.map_pose_last(camera=cam)[0]
    assert p["n_markers"] >= 2
    R, t = poses[10]
    print(f"end to end: a further frame's camera from its rendering pose: {np.linalg.norm(p['cam_t'] + R.T @ t) * 1000:.2f} mm")


def test_zz_print_the_largest_figures():
    print("largest over this run, in units of their bars:", WORST)
