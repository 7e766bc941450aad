"""The camera models of the pose kernels on the device (fid_camera and the _cam twins of include/fid_abi.h): the plumb-bob twins and
the rational model with zero extra coefficients against the calls that were there before (equal, not close), the device's
projection and its analytic Jacobian against the float64 NumPy statement of the three models and its complex-step derivative, poses
that give the generating pose back under rational, thin-prism and equidistant cameras, and the record of a fisheye marker that
cannot be posed.  Corners go straight to the calls; no images but the STag frames of pose_cases."""
import numpy as np
import pytest

import aruco_map_cases as mc
import camera_model_cases as cm
import pose_cases as pc
import stag_bundle_cases as bc
from fiducials_amd import stag as fstag
from fiducials_amd.camera import Camera
from fiducials_amd.detector import ArucoDetector

pytestmark = pytest.mark.gpu

NODE_LEN = 0.14


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=1, max_markers=32)
    yield d
    d.close()


def _lengths_as_override(lengths):
    distinct = sorted(set(float(v) for v in lengths))
    ids = np.array([distinct.index(float(v)) for v in lengths], dtype=np.int32)
    return ids, {i: v for i, v in enumerate(distinct)}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _cameras_equal_to(K, D5):
    """The cameras that must give the plumb-bob call's bits: its twin, and the rational model with 8 and 12 coefficients whose
    extra ones are zero."""
    D5 = np.asarray(D5, dtype=np.float64)
    return {"plumb_bob/5": Camera(cm.PLUMB_BOB, K, D5), "rational/8": Camera(cm.RATIONAL, K, np.concatenate([D5, np.zeros(3)])),
            "rational/12": Camera(cm.RATIONAL, K, np.concatenate([D5, np.zeros(7)]))}


# -------------------------------------------------------------------------------------------- nothing that exists moved
def test_plumb_bob_twins_are_the_old_calls(det):
    """fid_pose_cam with {PLUMB_BOB, 5} and with RATIONAL (8 and 12 coefficients, the extra ones zero) against fid_pose on every
    case of vga x mild and hd x barrel: rvec, tvec, image_error and object_error EQUAL.  The same on one frame each for
    fid_map_pose_cam, fid_stag_pose_last_cam, fid_stag_bundle_pose_cam and a 4-frame fid_stag_detect_markers_batch_cam call."""
    for cam, dist in (("vga", "mild"), ("hd", "barrel")):
        K, D = pc.camera_matrix(cam), pc.dist_coeffs(dist)
        cs = pc.cases_for(cam, dist)
        corners = np.stack([c.corners for c in cs])
        ids, override = _lengths_as_override([c.length for c in cs])
        old = det.estimate_pose_single_markers(corners, ids, NODE_LEN, K, D, override)
        assert np.isfinite(old.tvecs[list(pc.kept(cam, dist))]).all()
        for name, camera in _cameras_equal_to(K, D).items():
            new = det.estimate_pose_single_markers(corners, ids, NODE_LEN, fiducial_len_override=override, camera=camera)
            for field in ("rvecs", "tvecs", "image_error", "object_error"):
                assert _same(getattr(old, field), getattr(new, field)), (cam, dist, name, field)
    # ---- the camera among a map's fiducials
    name, Dv, R, t, P, exact, noisy = [c for c in mc.planar_cases() if np.any(c[1])][0]
    e = mc.planar_board(name)
    det.set_map(e)
    old = det.map_pose(mc.K, Dv, mc.split_markers(noisy), e["id"])
    assert old["n_markers"] == len(e)
    for cname, camera in _cameras_equal_to(mc.K, Dv).items():
        new = det.map_pose(corners=mc.split_markers(noisy), ids=e["id"], camera=camera)
        for field in old.dtype.names:
            assert _same(old[field], new[field]), ("map", cname, field)
    det.set_map(None)
    # ---- STag: the marker pose of one frame, the bundle pose of one hand-made frame, a batch of four frames
    K, D = pc.camera_matrix("vga"), pc.dist_coeffs("mild")
    sd = fstag.StagDetector(21, 7, max_width=640, max_height=480)
    try:
        n_markers, image = pc.stag_frames()[3]
        assert len(sd.detect_markers(image)) == n_markers
        old = sd.pose_last(K, D, 0.18)
        assert len(old) == n_markers
        for cname, camera in _cameras_equal_to(K, D).items():
            assert sd.pose_last(marker_size=0.18, camera=camera).tobytes() == old.tobytes(), ("stag pose", cname)
        sd.set_layout(fstag.board_layout(range(6), bc.oblique_board(6)))
        rng = np.random.default_rng(31)
        Pb = bc.tags_points(bc.oblique_board(6)[:4])
        Rb, tb = bc.seeded_pose(rng)
        img = bc.project(Pb, Rb, tb, bc.K, bc.D_NONZERO) + rng.uniform(-0.3, 0.3, size=(len(Pb), 2))
        m = bc.markers_from_points(range(4), img.reshape(4, 5, 2))
        old = sd.bundle_pose(bc.K, bc.D_NONZERO, m)
        assert len(old) == 1 and old["n_tags"][0] == 4
        for cname, camera in _cameras_equal_to(bc.K, bc.D_NONZERO).items():
            assert sd.bundle_pose(markers=m, camera=camera).tobytes() == old.tobytes(), ("stag bundle", cname)
        sd.set_layout(None)
    finally:
        sd.close()
    pool = fstag.StagPool(21, 7, n_contexts=4, max_width=640, max_height=480)
    try:
        frames = np.stack([im for _, im in pc.stag_frames()[:4]])
        om, op = pool.detect_markers_batch(frames, K, D, 0.18)
        assert [len(x) for x in om] == [n for n, _ in pc.stag_frames()[:4]]
        for cname, camera in _cameras_equal_to(K, D).items():
            nm, npo = pool.detect_markers_batch(frames, marker_size=0.18, camera=camera)
            for f in range(4):
                assert nm[f].tobytes() == om[f].tobytes() and npo[f].tobytes() == op[f].tobytes(), ("stag batch", cname, f)
    finally:
        pool.close()


# -------------------------------------------------------------------------------------------- projection and Jacobian
@pytest.mark.parametrize("cam", ["vga", "hd", "wide"])
@pytest.mark.parametrize("model", [cm.PLUMB_BOB, cm.RATIONAL, cm.EQUIDISTANT], ids=cm.model_name)
def test_projection_and_jacobian(det, model, cam):
    """fid_project_points_cam on 64 points: uv within 1e-9 px of the NumPy model, every Jacobian entry within 1e-9 x the largest
    magnitude of its row of the complex-step derivative of the NumPy model (both are float64 evaluations of one analytic
    expression: they differ by rounding; a wrong or missing term moves an entry by 1e-3 of its row or more)."""
    K, D = pc.camera_matrix(cam), cm.PROJECTION_SETS[model]
    rvec, tvec, pts = cm.projection_points(model, cam)
    assert len(pts) == 64
    uv, jac = det.project_points(Camera(model, K, D), rvec, tvec, pts, jacobian=True)
    want_uv = cm.project(model, K, D, rvec, tvec, pts)
    want_jac = cm.complex_step_jacobian(model, K, D, rvec, tvec, pts, 1e-30)
    duv = np.abs(uv - want_uv).max()
    rows = np.abs(want_jac).max(axis=2, keepdims=True)
    djac = (np.abs(jac - want_jac) / rows).max()
    print(f"\n{cm.model_name(model)} x {cam}: |duv| {duv:.3g} px, Jacobian {djac:.3g} of its row")
    assert np.array_equal(det.project_points(Camera(model, K, D), rvec, tvec, pts), uv)  # (without the Jacobian: the same points)
    assert duv <= 1e-9
    assert djac <= 1e-9


# -------------------------------------------------------------------------------------------- poses under the new models
@pytest.mark.parametrize("set_name", list(cm.SETS))
@pytest.mark.parametrize("cam", list(pc.CAMERAS))
def test_poses_recover_the_generating_pose(det, cam, set_name):
    """Every case of one camera x coefficient set in one fid_pose_cam call.  Kept cases (the zero-distortion twin is well-posed
    for the oracle; at most 5 % may be dropped): image_error <= 4 sigma^2 + 0.01 px^2; the noise-free ones give the generating
    pose back within five times the oracle's own deviation on this geometry (camera_model_cases.TOL_*).

    Measured on the device: camera_model_cases.DEVICE_MEASURED."""
    model, D = cm.SETS[set_name]
    K = pc.camera_matrix(cam)
    cs, keep = cm.cases_for(cam, set_name), cm.kept(cam, set_name)
    assert len(cs) - len(keep) <= cm.MAX_DROPPED * len(cs), (len(keep), len(cs))
    ids, override = _lengths_as_override([c.length for c in cs])
    pr = det.estimate_pose_single_markers(np.stack([c.corners for c in cs]), ids, NODE_LEN, fiducial_len_override=override, camera=Camera(model, K, D))
    worst_e, worst_t, worst_a, over = 0.0, 0.0, 0.0, []
    for i in keep:
        c = cs[i]
        e = float(pr.image_error[i])
        bound = 4.0 * c.sigma ** 2 + 0.01
        worst_e = max(worst_e, e - 4.0 * c.sigma ** 2)
        ok = np.isfinite(pr.rvecs[i]).all() and np.isfinite(pr.tvecs[i]).all() and 0.0 <= e <= bound
        if c.sigma == 0.0 and ok:
            dt = float(np.linalg.norm(pr.tvecs[i] - c.tvec) / np.linalg.norm(c.tvec))
            da = pc.rotation_angle(pc.rodrigues(pr.rvecs[i]) @ c.R.T)
            worst_t, worst_a = max(worst_t, dt), max(worst_a, da)
            ok = dt <= cm.TOL_DT_REL and da <= cm.TOL_DANGLE
        if not ok:
            over.append((i, c.length, c.side, c.tilt, c.sigma, e, pr.rvecs[i].tolist(), pr.tvecs[i].tolist(), c.tvec.tolist()))
    print(f"\n{cam} x {set_name}: {len(keep)} of {len(cs)} kept; image_error - 4 sigma^2 <= {worst_e:.3g} px^2; noise-free: |dt|/|t| {worst_t:.3g} "
          f"(tolerance {cm.TOL_DT_REL:.3g}), angle {worst_a:.3g} rad (tolerance {cm.TOL_DANGLE:.3g})")
    assert not over, (len(over), over[:4])


def test_fisheye_marker_beyond_the_model_is_reported(det):
    """A marker whose corners lie at theta_d past 89 degrees gets rvec = tvec = 0 and image_error = -1; its neighbours in the same
    call are posed as they are without it."""
    cam, set_name = "vga", "fe_mild"
    model, D = cm.SETS[set_name]
    fx, fy, cx, cy, _, _ = pc.CAMERAS[cam]
    camera = Camera(model, pc.camera_matrix(cam), D)
    cs, keep = cm.cases_for(cam, set_name), cm.kept(cam, set_name)
    good = [cs[i] for i in keep if cs[i].length == NODE_LEN][:2]
    assert len(good) == 2
    # a 60 px square whose nearest corner is 1.58 rad (90.5 degrees) from the axis
    u0 = cx + 1.58 * fx
    beyond = np.array([[u0, 200.0], [u0 + 60.0, 200.0], [u0 + 60.0, 260.0], [u0, 260.0]], dtype=np.float32)
    assert (np.hypot((beyond[:, 0] - cx) / fx, (beyond[:, 1] - cy) / fy) > np.deg2rad(89.0)).all()
    ids = np.zeros(3, np.int32)
    pr = det.estimate_pose_single_markers(np.stack([good[0].corners, beyond, good[1].corners]), ids, NODE_LEN, camera=camera)
    alone = det.estimate_pose_single_markers(np.stack([good[0].corners, good[1].corners]), ids[:2], NODE_LEN, camera=camera)
    assert np.array_equal(pr.rvecs[1], np.zeros(3)) and np.array_equal(pr.tvecs[1], np.zeros(3)) and pr.image_error[1] == -1.0
    for a, b in ((0, 0), (2, 1)):
        assert np.array_equal(pr.rvecs[a], alone.rvecs[b]) and np.array_equal(pr.tvecs[a], alone.tvecs[b]) and pr.image_error[a] == alone.image_error[b]
        assert 0.0 <= pr.image_error[a] <= 4.0 * good[b].sigma ** 2 + 0.01
        assert np.linalg.norm(pr.tvecs[a] - good[b].tvec) / np.linalg.norm(good[b].tvec) < 1e-2
