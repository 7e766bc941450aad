"""The pose covariance on the device (include/fid_abi.h, "pose covariance"; the _cov entry points) against the float64 NumPy statement
of pose_cov_cases.py, evaluated at the DEVICE's own pose: cov_rt, cov_pose and cov_cam_pose within pose_cov_cases.tol() as whitened
deviations, the pose records equal to the twins', exact symmetry, the exact factor 4 between sigma_px 2 and 1, the a-posteriori
variance, the refused sigmas, the record of a pose that is not there, and the remembered road through fid_detect / fid_submit_batch.

Measured on the device: pose_cov_cases.DEVICE_MEASURED."""
import ctypes as C

import numpy as np
import pytest

import aruco_map_cases as mc
import camera_model_cases as cm
import pose_cases as pc
import pose_cov_cases as cc
import stag_bundle_cases as bc
from fiducials_amd import _lib
from fiducials_amd import stag as fstag
from fiducials_amd import synth
from fiducials_amd.camera import Camera
from fiducials_amd.detector import MAP_POSE_COV_DTYPE, POSE_COV_DTYPE, ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary

pytestmark = pytest.mark.gpu

W, H = 640, 480
MATS = ("cov_rt", "cov_pose")


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(mc.DICT, max_width=W, max_height=H, max_batch=2, max_markers=4)
    yield d
    d.close()


@pytest.fixture(scope="module")
def sdet():
    d = fstag.StagDetector(21, 7, max_width=W, max_height=H)
    yield d
    d.close()


@pytest.fixture(scope="module")
def tol():
    return cc.tol()


def _symmetric(m) -> bool:
    return np.array_equal(m, np.swapaxes(m, -1, -2))


def _check_record(rec, model, K, D, rvec, tvec, obj, img, sigma_px, tol, what):
    """One valid fid_pose_cov against the reference at (rvec, tvec); returns the larger whitened deviation."""
    assert rec["status"] == 0 and rec["n_points"] == len(obj), (what, rec["status"], rec["n_points"])
    c_rt, c_pose, s2 = cc.reference_cov(model, K, D, rvec, tvec, obj, img, sigma_px)
    assert abs(rec["sigma2"] - s2) <= 1e-9 * s2, (what, rec["sigma2"], s2)
    devs = (cc.whitened_dev(rec["cov_rt"], c_rt), cc.whitened_dev(rec["cov_pose"], c_pose))
    print(f"{what}: cov_rt {devs[0]:.3g}, cov_pose {devs[1]:.3g} (TOL {tol:.3g})")
    assert max(devs) <= tol, (what, devs)
    assert _symmetric(rec["cov_rt"]) and _symmetric(rec["cov_pose"]), what
    return max(devs)


# -------------------------------------------------------------------------------------------- k_pose
@pytest.mark.parametrize("set_name", list(cc.CAMERA_SETS))
def test_marker_pose_covariance(det, tol, set_name):
    """fid_pose_cov_cam on the four markers of the cases (a length override, small and far, large and oblique, the second frame's)
    under one camera set: the poses are fid_pose_cam's bytes; every matrix against the reference at the device's pose; symmetry;
    sigma_px = 2 is four times sigma_px = 1, exactly."""
    model, D = cc.CAMERA_SETS[set_name]
    K = pc.camera_matrix(cc.CAM)
    camera = Camera(model, K, D)
    ids, lens, corners, objs, _, _ = cc.marker_cases(set_name)
    override = {int(ids[0]): cc.OVERRIDE_LEN}
    twin = det.estimate_pose_single_markers(corners, ids, cc.NODE_LEN, fiducial_len_override=override, camera=camera)
    pr, cov = det.estimate_pose_single_markers_cov(corners, ids, cc.NODE_LEN, fiducial_len_override=override, camera=camera, sigma_px=1.0)
    pr2, cov2 = det.estimate_pose_single_markers_cov(corners, ids, cc.NODE_LEN, fiducial_len_override=override, camera=camera, sigma_px=2.0)
    for field in ("rvecs", "tvecs", "image_error", "object_error", "fiducial_area"):
        assert np.array_equal(getattr(pr, field), getattr(twin, field)) and np.array_equal(getattr(pr2, field), getattr(twin, field)), field
    print()
    for k in range(4):
        _check_record(cov[k], model, K, D, pr.rvecs[k], pr.tvecs[k], objs[k], corners[k], 1.0, tol, f"{set_name} marker {k}")
    for m in MATS:
        assert np.array_equal(cov2[m], 4.0 * cov[m]), m
    assert np.array_equal(cov2["sigma2"], 4.0 * cov["sigma2"])
    # the small far marker is the poorly determined one, the large oblique one is pinned down: depth sigma in units of the depth
    rel = [np.sqrt(cov[k]["cov_pose"][2, 2]) / pr.tvecs[k][2] for k in (1, 2)]
    assert rel[0] > 10.0 * rel[1], rel


def test_a_posteriori_variance(det, tol):
    """sigma_px = 0 on noisy corners: sigma2 = |e|^2 / (2 N - 6) from NumPy at the device's pose to 1e-9, and cov_rt = sigma2 x the
    unit-variance matrix within TOL."""
    model, D = cc.CAMERA_SETS["prism12"]
    K = pc.camera_matrix(cc.CAM)
    camera = Camera(model, K, D)
    ids, lens, corners, objs, _, _ = cc.marker_cases("prism12", True)
    override = {int(ids[0]): cc.OVERRIDE_LEN}
    pr, cov0 = det.estimate_pose_single_markers_cov(corners, ids, cc.NODE_LEN, fiducial_len_override=override, camera=camera, sigma_px=0.0)
    pr1, cov1 = det.estimate_pose_single_markers_cov(corners, ids, cc.NODE_LEN, fiducial_len_override=override, camera=camera, sigma_px=1.0)
    assert np.array_equal(pr.rvecs, pr1.rvecs) and np.array_equal(pr.tvecs, pr1.tvecs)
    print()
    for k in range(4):
        _, e2 = cc.normal_matrix(model, K, D, pr.rvecs[k], pr.tvecs[k], objs[k], corners[k])
        want = e2 / (2 * 4 - 6)
        assert want > 1e-6, want  # (noisy corners: not a variance of rounding)
        assert abs(cov0[k]["sigma2"] - want) <= 1e-9 * want, (k, cov0[k]["sigma2"], want)
        assert cc.whitened_dev(cov0[k]["cov_rt"], cov0[k]["sigma2"] * cov1[k]["cov_rt"]) <= tol
        _check_record(cov0[k], model, K, D, pr.rvecs[k], pr.tvecs[k], objs[k], corners[k], 0.0, tol, f"a-posteriori marker {k}")


def test_refused_sigma_leaves_the_output_untouched(det):
    model, D = cc.CAMERA_SETS["barrel"]
    camera = Camera(model, pc.camera_matrix(cc.CAM), D)
    ids, _, corners, _, _, _ = cc.marker_cases("barrel")
    for bad in (-1.0, float("nan"), float("inf")):
        mk = (_lib.FidMarker * 4)()
        for i in range(4):
            mk[i].id = int(ids[i])
            for j in range(8):
                mk[i].corners[j] = float(corners[i].reshape(8)[j])
        out = (_lib.FidPoseOut * 4)()
        before = bytes(out)
        cov = np.full(4, 7, np.uint8).repeat(POSE_COV_DTYPE.itemsize).view(POSE_COV_DTYPE)
        cov_before = cov.tobytes()
        rc = det._L.fid_pose_cov_cam(det._ctx, C.byref(camera.c), mk, None, 4, cc.NODE_LEN, out, bad, cov.ctypes.data)
        assert rc == _lib.FID_E_INVALID_ARG, (bad, rc)
        assert bytes(out) == before and cov.tobytes() == cov_before, bad


def test_unposable_fisheye_marker_has_status_1(det, tol):
    """The equidistant model's "cannot be posed" record: status 1 and zeros; its neighbours in the same call stay valid and are what
    they are without it."""
    model, D = cm.SETS["fe_mild"]
    fx, fy, cx, cy, _, _ = pc.CAMERAS["vga"]
    K = pc.camera_matrix("vga")
    camera = Camera(model, K, D)
    cs, keep = cm.cases_for("vga", "fe_mild"), cm.kept("vga", "fe_mild")
    good = [cs[i] for i in keep if cs[i].length == cc.NODE_LEN and cs[i].sigma == 0.0][:2]
    u0 = cx + 1.58 * fx
    beyond = np.array([[u0, 200.0], [u0 + 60.0, 200.0], [u0 + 60.0, 260.0], [u0, 260.0]], dtype=np.float32)
    ids = np.zeros(3, np.int32)
    pr, cov = det.estimate_pose_single_markers_cov(np.stack([good[0].corners, beyond, good[1].corners]), ids, cc.NODE_LEN, camera=camera)
    alone, cov_alone = det.estimate_pose_single_markers_cov(np.stack([good[0].corners, good[1].corners]), ids[:2], cc.NODE_LEN, camera=camera)
    assert pr.image_error[1] == -1.0 and cov[1]["status"] == 1 and cov[1]["sigma2"] == 0.0
    assert not cov[1]["cov_rt"].any() and not cov[1]["cov_pose"].any()
    obj = pc.square_object_points(cc.NODE_LEN)
    print()
    for a, b in ((0, 0), (2, 1)):
        assert cov[a].tobytes() == cov_alone[b].tobytes()
        _check_record(cov[a], model, K, D, pr.rvecs[a], pr.tvecs[a], obj, good[b].corners, 1.0, tol, f"fisheye neighbour {a}")


# -------------------------------------------------------------------------------------------- k_stag_pose
def _stag_frame_markers(sdet):
    """Two markers of a rendered STag frame in the context (fid_stag_pose_last* poses the last detect call's markers)."""
    n_markers, image = pc.stag_frames()[1]
    m = sdet.detect_markers(image)
    assert len(m) == n_markers >= 2
    return m


def test_stag_marker_pose_covariance(sdet, tol):
    """fid_stag_pose_last_cov_cam on the markers of one rendered frame (the 5-point record): the poses are fid_stag_pose_last_cam's
    bytes, the first two markers' matrices against the reference at the device's pose over the centre and the four corners."""
    m = _stag_frame_markers(sdet)
    camera = Camera(cm.PLUMB_BOB, cc.STAG_K, cc.STAG_D)
    twin = sdet.pose_last(marker_size=cc.STAG_SIZE, camera=camera)
    poses, cov = sdet.pose_cov_last(marker_size=cc.STAG_SIZE, camera=camera, sigma_px=1.0)
    poses2, cov2 = sdet.pose_cov_last(marker_size=cc.STAG_SIZE, camera=camera, sigma_px=2.0)
    assert poses.tobytes() == twin.tobytes() == poses2.tobytes() and len(cov) == len(m)
    obj = pc.stag_object_points(cc.STAG_SIZE)
    print()
    for k in range(2):
        img = np.concatenate([m["center"][k][None], m["corners"][k]])
        _check_record(cov[k], cm.PLUMB_BOB, cc.STAG_K, cc.STAG_D, poses["rvec"][k], poses["tvec"][k], obj, img, 1.0, tol, f"stag marker {k}")
    for f in MATS:
        assert np.array_equal(cov2[f], 4.0 * cov[f]), f
    assert sdet.pose_last(marker_size=cc.STAG_SIZE, camera=camera).tobytes() == twin.tobytes()


# -------------------------------------------------------------------------------------------- k_stag_bundle_pose
def test_stag_bundle_pose_covariance(sdet, tol):
    """fid_stag_bundle_pose_cov_cam on hand-made markers: a coplanar 2-tag bundle, a 2-tag bundle on two faces, and a third bundle
    of which no tag is among the markers (no record, as in the twin); then the same markers without the first bundle's, where the
    records keep the twin's indexing."""
    boards, posed = cc.bundle_cases()
    tags = []
    for b, (board, first_id) in enumerate(zip(boards, (0, 2, 4))):
        tags += [fstag.tag_from_three_corners(first_id + k, b, c[0], c[1], c[2]) for k, c in enumerate(board)]
    sdet.set_layout(fstag.Layout(np.array(tags, dtype=fstag.TAG_DTYPE), ["flat", "faces", "absent"], np.zeros(3, bool)))
    try:
        camera = Camera(cm.PLUMB_BOB, bc.K, bc.D_NONZERO)
        ms = np.concatenate([bc.markers_from_points((0, 1), posed[0][1].reshape(2, 5, 2)), bc.markers_from_points((2, 3), posed[1][1].reshape(2, 5, 2))])
        twin = sdet.bundle_pose(markers=ms, camera=camera)
        got, cov = sdet.bundle_pose_cov(markers=ms, camera=camera, sigma_px=1.0)
        got2, cov2 = sdet.bundle_pose_cov(markers=ms, camera=camera, sigma_px=2.0)
        assert got.tobytes() == twin.tobytes() == got2.tobytes()
        assert list(got["bundle"]) == [0, 1] and list(got["n_tags"]) == [2, 2] and len(cov) == 2
        print()
        for b in range(2):
            P, img, _, _ = posed[b]
            _check_record(cov[b], cm.PLUMB_BOB, bc.K, bc.D_NONZERO, got["rvec"][b], got["tvec"][b], P, img, 1.0, tol, f"bundle {b}")
        for f in MATS:
            assert np.array_equal(cov2[f], 4.0 * cov[f]), f
        only, cov_only = sdet.bundle_pose_cov(markers=ms[2:], camera=camera, sigma_px=1.0)
        assert list(only["bundle"]) == [1] and only.tobytes() == got[1:].tobytes() and cov_only.tobytes() == cov[1:].tobytes()
        none, cov_none = sdet.bundle_pose_cov(markers=bc.markers_from_points((9,), posed[0][1].reshape(2, 5, 2)[:1]), camera=camera)
        assert len(none) == 0 and len(cov_none) == 0
    finally:
        sdet.set_layout(None)


# -------------------------------------------------------------------------------------------- k_map_pose
def test_map_pose_covariance(det, tol):
    """fid_map_pose_cov_cam: a 4-marker board of which 3 are seen -- cov, cov_pose and cov_cam_pose against the reference at the
    device's pose --, and a frame in which no marker is mapped (status 1, zeros)."""
    e, seen, P, img, _, _ = cc.map_case()
    camera = Camera(cm.PLUMB_BOB, mc.K, mc.D_NONZERO)
    det.set_map(e)
    try:
        corners = mc.split_markers(img)
        twin = det.map_pose(corners=corners, ids=e["id"][seen], camera=camera)
        got, cov = det.map_pose_cov(corners=corners, ids=e["id"][seen], camera=camera, sigma_px=1.0)
        got2, cov2 = det.map_pose_cov(corners=corners, ids=e["id"][seen], camera=camera, sigma_px=2.0)
        assert got.tobytes() == twin.tobytes() == got2.tobytes() and got["n_markers"] == 3
        print()
        img32 = corners.reshape(-1, 2).astype(np.float64)
        _check_record(cov["pose"], cm.PLUMB_BOB, mc.K, mc.D_NONZERO, got["rvec"], got["tvec"], P, img32, 1.0, tol, "map pose")
        want_cam = cc.reference_cov_cam(got["rvec"], got["tvec"], cc.reference_cov(cm.PLUMB_BOB, mc.K, mc.D_NONZERO, got["rvec"], got["tvec"], P, img32, 1.0)[1])
        dev = cc.whitened_dev(cov["cov_cam_pose"], want_cam)
        print(f"map pose: cov_cam_pose {dev:.3g}")
        assert dev <= tol and _symmetric(cov["cov_cam_pose"])
        for f in ("cov_rt", "cov_pose"):
            assert np.array_equal(cov2["pose"][f], 4.0 * cov["pose"][f]), f
        assert np.array_equal(cov2["cov_cam_pose"], 4.0 * cov["cov_cam_pose"])
        # no marker of the frame is in the map
        none, cov_none = det.map_pose_cov(corners=corners[:1], ids=np.array([77], np.int32), camera=camera)
        assert none["n_markers"] == 0 and none.tobytes() == det.map_pose(corners=corners[:1], ids=np.array([77], np.int32), camera=camera).tobytes()
        assert cov_none["pose"]["status"] == 1 and not cov_none["pose"]["cov_rt"].any() and not cov_none["pose"]["cov_pose"].any()
        assert not cov_none["cov_cam_pose"].any()
    finally:
        det.set_map(None)


# -------------------------------------------------------------------------------------------- the remembered road
def _frames():
    d = get_predefined_dictionary(mc.DICT)
    return [synth.make_frame(d, seed=s, width=W, height=H, n_markers=n, side_range=(60, 110)) for s, n in ((7, 4), (8, 3), (9, 1))]


def test_remembered_road(det, tol):
    """fid_pose_last_cov_cam after fid_detect; a second fid_detect of the same frame then runs the covariance form in its own stream
    and the call after it is a copy: the same bytes; fid_pose_last_cam after that returns its usual bytes; the same once through
    fid_submit_batch / fid_collect with 2 frames of 3 and 1 markers at cap 4 (the per-frame stride and a dead group), where a _cov call
    while the batch is in flight is refused (fid_map_pose_last_cov_cam too; its own road: test_map_pose_covariance_of_a_two_frame_batch)."""
    f4, f3, f1 = _frames()
    K = np.array([[1400.0 * W / 1920.0, 0, W / 2.0], [0, 1400.0 * W / 1920.0, H / 2.0], [0, 0, 1.0]])
    camera = Camera(cm.PLUMB_BOB, K, pc.dist_coeffs("mild"))
    other = ArucoDetector(mc.DICT, max_width=W, max_height=H, max_batch=2, max_markers=4)
    try:
        corners, ids = other.detect_markers(f4.image)
        assert len(ids) == 4
        usual = other.pose_last(cc.NODE_LEN, camera=camera, unpack=True)[0]  # a context that never asks for a covariance
        corners, ids = det.detect_markers(f4.image)
        p1, c1 = det.pose_cov_last(cc.NODE_LEN, camera=camera, sigma_px=1.0)  # 1
        det.detect_markers(f4.image)
        p2, c2 = det.pose_cov_last(cc.NODE_LEN, camera=camera, sigma_px=1.0)  # 2: computed in the detect call's stream
        assert len(c1[0]) == 4 and c1[0].tobytes() == c2[0].tobytes()
        for field in ("rvecs", "tvecs", "image_error", "object_error", "fiducial_area"):
            assert np.array_equal(getattr(p1[0], field), getattr(p2[0], field)) and np.array_equal(getattr(p1[0], field), getattr(usual, field)), field
        p3 = det.pose_last(cc.NODE_LEN, camera=camera)[0]  # 3
        for field in ("rvecs", "tvecs", "image_error", "object_error", "fiducial_area"):
            assert np.array_equal(getattr(p3, field), getattr(usual, field)), field
        obj = pc.square_object_points(cc.NODE_LEN)
        print()
        for k in range(4):
            _check_record(c1[0][k], cm.PLUMB_BOB, K, pc.dist_coeffs("mild"), p1[0].rvecs[k], p1[0].tvecs[k], obj, corners[k], 1.0, tol, f"detected marker {k}")
        # 4: a batch of two frames with 3 and 1 markers at cap 4, submitted and collected
        batch = np.ascontiguousarray(np.stack([f3.image, f1.image]))
        det.submit_batch(batch)
        cov = np.zeros(8, POSE_COV_DTYPE)
        rc = det._L.fid_pose_last_cov_cam(det._ctx, C.byref(camera.c), cc.NODE_LEN, det._poses, 4, 1.0, cov.ctypes.data)
        assert rc == _lib.FID_E_INVALID_ARG
        mcov = np.zeros(2, MAP_POSE_COV_DTYPE)
        mout = np.zeros(2, np.uint8).repeat(512)
        assert det._L.fid_map_pose_last_cov_cam(det._ctx, C.byref(camera.c), mout.ctypes.data, 2, 1.0, mcov.ctypes.data) == _lib.FID_E_INVALID_ARG
        found = det.collect()
        assert [len(i) for _, i in found] == [3, 1]
        pb, cb = det.pose_cov_last(cc.NODE_LEN, camera=camera, sigma_px=1.0)  # (a copy: the batch ran k_pose_cov in its stream)
        assert [len(c) for c in cb] == [3, 1]
        for f in range(2):
            one = ArucoDetector(mc.DICT, max_width=W, max_height=H, max_batch=1, max_markers=4)
            try:
                cs, _ = one.detect_markers(batch[f])
                assert np.array_equal(cs, found[f][0])
                q, cq = one.pose_cov_last(cc.NODE_LEN, camera=camera, sigma_px=1.0)
            finally:
                one.close()
            assert cb[f].tobytes() == cq[0].tobytes() and np.array_equal(pb[f].rvecs, q[0].rvecs) and np.array_equal(pb[f].tvecs, q[0].tvecs)
            for k in range(len(cb[f])):
                _check_record(cb[f][k], cm.PLUMB_BOB, K, pc.dist_coeffs("mild"), pb[f].rvecs[k], pb[f].tvecs[k], obj, found[f][0][k], 1.0, tol, f"batch frame {f} marker {k}")
    finally:
        other.close()


def test_remembered_road_of_the_map_pose(tol):
    """fid_map_pose_last_cov_cam on a rendered scene: computed behind the detect call the first time, in its stream the second
    time; the same bytes, map_pose_last's record unchanged."""
    name, pose = "2x2", 1
    fr = mc.scene(name, pose)
    camera = Camera(cm.PLUMB_BOB, mc.K, np.zeros(5))
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=1, max_markers=16)
    try:
        d.set_map(mc.scene_map(name))
        corners, ids = d.detect_markers(fr.image)
        usual = d.map_pose_last(camera=camera)
        m1, c1 = d.map_pose_cov_last(camera=camera, sigma_px=1.0)
        d.detect_markers(fr.image)
        m2, c2 = d.map_pose_cov_last(camera=camera, sigma_px=1.0)
        assert m1.tobytes() == usual.tobytes() == m2.tobytes() and c1.tobytes() == c2.tobytes()
        assert d.map_pose_last(camera=camera).tobytes() == usual.tobytes()
        assert m1["n_markers"][0] == len(ids) and c1["pose"]["status"][0] == 0
        P = mc.map_points_for(mc.scene_map(name), ids)
        img = corners.reshape(-1, 2).astype(np.float64)
        print()
        _check_record(c1["pose"][0], cm.PLUMB_BOB, mc.K, np.zeros(5), m1["rvec"][0], m1["tvec"][0], P, img, 1.0, tol, "scene map pose")
        want_cam = cc.reference_cov_cam(m1["rvec"][0], m1["tvec"][0], cc.reference_cov(cm.PLUMB_BOB, mc.K, np.zeros(5), m1["rvec"][0], m1["tvec"][0], P, img, 1.0)[1])
        assert cc.whitened_dev(c1["cov_cam_pose"][0], want_cam) <= tol
    finally:
        d.close()


def test_map_pose_covariance_of_a_two_frame_batch(tol):
    """k_map_pose's COV form on more than one frame: a batch of a rendered 4-marker board of which 3 are in the picture and a frame
    whose only marker the map does not name.  Frame 0 against the reference at the device's pose and against a one-frame context,
    byte for byte; frame 1 status 1 with zeros in all three matrices beside it.  First computed behind the batch, then (a second
    batch, submitted and collected) in its stream: the same bytes."""
    name, pose = "2x2", 1
    emap = mc.scene_map(name)
    fr = mc.scene(name, pose, without=2)
    stranger = int(max(emap["id"])) + 17
    other = synth.make_frame(get_predefined_dictionary(mc.DICT), seed=9, width=mc.W, height=mc.H, n_markers=1, ids=np.array([stranger]), side_range=(60, 110))
    batch = np.ascontiguousarray(np.stack([fr.image, other.image]))
    camera = Camera(cm.PLUMB_BOB, mc.K, pc.dist_coeffs("mild"))
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=2, max_markers=16)
    one = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=1, max_markers=16)
    try:
        d.set_map(emap)
        one.set_map(emap)
        found = d.detect_markers_batch(batch)
        assert len(found[0][1]) == 3 and list(found[1][1]) == [stranger]
        usual = d.map_pose_last(camera=camera)
        m1, c1 = d.map_pose_cov_last(camera=camera, sigma_px=1.0)
        d.submit_batch(batch)
        d.collect()
        m2, c2 = d.map_pose_cov_last(camera=camera, sigma_px=1.0)  # (a copy: the batch ran the COV form in its stream)
        assert len(m1) == 2 and m1.tobytes() == usual.tobytes() == m2.tobytes() and c1.tobytes() == c2.tobytes()
        # frame 0: three mapped markers
        assert m1["n_markers"][0] == 3 and c1["pose"]["status"][0] == 0
        one.detect_markers(batch[0])
        mo, co = one.map_pose_cov_last(camera=camera, sigma_px=1.0)
        assert mo.tobytes() == m1[:1].tobytes() and co.tobytes() == c1[:1].tobytes()
        P = mc.map_points_for(emap, found[0][1])
        img = found[0][0].reshape(-1, 2).astype(np.float64)
        D = pc.dist_coeffs("mild")
        print()
        _check_record(c1["pose"][0], cm.PLUMB_BOB, mc.K, D, m1["rvec"][0], m1["tvec"][0], P, img, 1.0, tol, "batch frame 0 map pose")
        want_cam = cc.reference_cov_cam(m1["rvec"][0], m1["tvec"][0], cc.reference_cov(cm.PLUMB_BOB, mc.K, D, m1["rvec"][0], m1["tvec"][0], P, img, 1.0)[1])
        dev = cc.whitened_dev(c1["cov_cam_pose"][0], want_cam)
        print(f"batch frame 0 map pose: cov_cam_pose {dev:.3g}")
        assert dev <= tol and _symmetric(c1["cov_cam_pose"][0])
        # frame 1: a marker, none mapped
        assert m1["n_markers"][1] == 0 and c1["pose"]["status"][1] == 1 and c1["pose"]["sigma2"][1] == 0.0
        assert not c1["pose"]["cov_rt"][1].any() and not c1["pose"]["cov_pose"][1].any() and not c1["cov_cam_pose"][1].any()
        assert d.map_pose_last(camera=camera).tobytes() == usual.tobytes()
    finally:
        d.close()
        one.close()


BAD_SIGMAS = (-1.0, float("nan"), float("inf"))


def test_every_cov_entry_point_refuses_a_bad_sigma(sdet):
    """The six entry points beside fid_pose_cov_cam: with a usable sigma_px the call succeeds; with -1, NaN or inf it returns
    FID_E_INVALID_ARG and leaves the pose array and the covariance array as they were."""
    fr = mc.scene("2x2", 1)
    camera = Camera(cm.PLUMB_BOB, mc.K, np.zeros(5))
    cam = C.byref(camera.c)
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=1, max_markers=16)
    try:
        d.set_map(mc.scene_map("2x2"))
        corners, ids = d.detect_markers(fr.image)
        mk = np.zeros(len(ids), np.dtype([("id", "<i4"), ("corners", "<f4", (8,))]))
        mk["id"], mk["corners"] = ids, corners.reshape(-1, 8)
        L, ctx = d._L, d._ctx
        calls = {
            "fid_pose_last_cov_cam": (16 * 72, 16 * POSE_COV_DTYPE.itemsize, lambda o, c, s: L.fid_pose_last_cov_cam(ctx, cam, cc.NODE_LEN, C.cast(C.c_void_p(o), C.POINTER(_lib.FidPoseOut)), 16, s, c)),
            "fid_map_pose_last_cov_cam": (512, MAP_POSE_COV_DTYPE.itemsize, lambda o, c, s: L.fid_map_pose_last_cov_cam(ctx, cam, o, 1, s, c)),
            "fid_map_pose_cov_cam": (512, MAP_POSE_COV_DTYPE.itemsize, lambda o, c, s: L.fid_map_pose_cov_cam(ctx, cam, mk.ctypes.data, len(mk), o, s, c)),
        }
        _refusals(calls)
    finally:
        d.close()
    boards, posed = cc.bundle_cases()
    tags = [fstag.tag_from_three_corners(k, 0, c[0], c[1], c[2]) for k, c in enumerate(boards[0])]
    n_markers, image = pc.stag_frames()[1]
    assert len(sdet.detect_markers(image)) == n_markers
    sdet.set_layout(fstag.Layout(np.array(tags, dtype=fstag.TAG_DTYPE), ["flat"], np.zeros(1, bool)))
    try:
        scam = C.byref(Camera(cm.PLUMB_BOB, bc.K, bc.D_NONZERO).c)
        ms = bc.markers_from_points((0, 1), posed[0][1].reshape(2, 5, 2))
        L, ctx = sdet._L, sdet._ctx
        n = C.c_int32(0)
        nb = fstag.MAX_BUNDLES
        calls = {
            "fid_stag_pose_last_cov_cam": (64 * fstag.POSE_DTYPE.itemsize, 64 * POSE_COV_DTYPE.itemsize,
                                           lambda o, c, s: L.fid_stag_pose_last_cov_cam(ctx, scam, cc.STAG_SIZE, o, 64, C.byref(n), s, c)),
            "fid_stag_bundle_pose_last_cov_cam": (nb * fstag.BUNDLE_POSE_DTYPE.itemsize, nb * POSE_COV_DTYPE.itemsize,
                                                  lambda o, c, s: L.fid_stag_bundle_pose_last_cov_cam(ctx, scam, o, nb, C.byref(n), s, c)),
            "fid_stag_bundle_pose_cov_cam": (nb * fstag.BUNDLE_POSE_DTYPE.itemsize, nb * POSE_COV_DTYPE.itemsize,
                                             lambda o, c, s: L.fid_stag_bundle_pose_cov_cam(ctx, scam, ms.ctypes.data, len(ms), o, nb, C.byref(n), s, c)),
        }
        _refusals(calls)
    finally:
        sdet.set_layout(None)


def _refusals(calls):
    for name, (out_bytes, cov_bytes, call) in calls.items():
        out, cov = np.full(out_bytes, 7, np.uint8), np.full(cov_bytes, 7, np.uint8)
        assert call(out.ctypes.data, cov.ctypes.data, 1.0) == _lib.FID_OK, name
        for bad in BAD_SIGMAS:
            out[:], cov[:] = 7, 7
            assert call(out.ctypes.data, cov.ctypes.data, bad) == _lib.FID_E_INVALID_ARG, (name, bad)
            assert (out == 7).all() and (cov == 7).all(), (name, bad)
