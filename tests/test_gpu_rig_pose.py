"""One rig pose per time step from all cameras of a rig on the device (k_rig_pose, fid_set_rig, fid_rig_pose, fid_rig_pose_last):
a one-camera rig against fid_map_pose, the kernel against its NumPy restatement (tests/rig_restatement.py) on hand-made marker sets
of rig_cases, against the exact minimum, the gather rules, the start camera, determinism and batches, rendered frames end to end,
the covariance, and what the entry points refuse.

The bound of the comparison with the exact minimiser (NumPy Gauss-Newton on the joint residuals with the analytic Jacobian, started
from the truth, run to a step below 1e-14) is not chosen: CvLevMarq ends at 20 steps / FLT_EPSILON, not at the minimum, so the
distance between the RESTATEMENT and that minimiser is measured on the CPU over the noisy cases (rig_cases.gap_to_minimum: 3.7e-10
when this file was written) and ten times the largest such distance is allowed (FACTOR)."""
import numpy as np
import pytest

import aruco_map_cases as mc
import pose_cov_cases as cc
import rig_cases as rc
import rig_restatement as rr
from fiducials_amd import _lib, synth
from fiducials_amd.camera import Camera, RigCamera
from fiducials_amd.detector import MAP_POSE_COV_DTYPE, RIG_POSE_DTYPE, ArucoDetector, FidError

pytestmark = pytest.mark.gpu

FACTOR = 10.0
INT_FIELDS = ("n_markers", "n_cameras", "n_over", "n_unposable", "start_camera")


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=8, max_markers=32)
    yield d
    d.close()


def _run(det, c, sigma_px=None):
    det.set_map(c.entries)
    det.set_rig(rc.lib_rig(c.cams))
    return det.rig_pose(c.corners, c.ids, sigma_px)


def _check_record(got):
    assert got["reserved0"] == 0
    assert np.abs(got["R"] - synth._rodrigues(got["rvec"])).max() < 1e-12
    assert np.abs(got["rig_R"] - got["R"].T).max() < 1e-12 and np.abs(got["rig_t"] + got["R"].T @ got["tvec"]).max() < 1e-12


def _same_integers(got, want):
    for f in INT_FIELDS:
        assert int(got[f]) == int(want[f]), (f, int(got[f]), int(want[f]))
    assert got["n_per_camera"].tolist() == list(want["n_per_camera"])


# ------------------------------------------------------------------------------------------------ 1. reduces to what exists
@pytest.mark.parametrize("rig", ["identity", "moved"])
def test_a_one_camera_rig_is_the_map_pose(det, rig):
    """Planar boards (aruco_map_cases.planar_cases) and two walls at right angles: with identity extrinsics R, tvec equal fid_map_pose's
    record for the same markers to 1e-6; with an extrinsic, that camera pose composed with it."""
    cam = (rc.RIG1_IDENTITY if rig == "identity" else rc.RIG1_MOVED)[0]
    det.set_rig(rc.lib_rig([cam]))
    sets = [(mc.planar_board(name), Dv, noisy) for name, Dv, _, _, _, _, noisy in mc.planar_cases() if Dv.any()]
    e = mc.corner_of_two_walls(3, 3)
    rng = np.random.default_rng(33)
    for _ in range(2):
        eye = np.array([0.2, 0.0, 0.2]) + rng.uniform(0.7, 1.1) * synth._rodrigues(rng.uniform(-0.25, 0.25, 3)) @ np.array([0.7, 0.1, 0.7])
        R, t = mc.look_at(eye, [0.2, 0.0, 0.2])
        img = mc.project(mc.object_points(e), R, t, mc.K, mc.D_NONZERO) + rng.uniform(-mc.NOISE_PX, mc.NOISE_PX, (24, 2))
        sets.append((e, mc.D_NONZERO, img.astype(np.float32).astype(np.float64)))
    worst = 0.0
    for entries, Dv, img in sets:
        det.set_map(entries)
        corners = mc.split_markers(img)
        one = det.map_pose(mc.K, Dv, corners, entries["id"])
        got = det.rig_pose([corners], [entries["id"]])
        assert got["n_markers"] == one["n_markers"] == len(entries) and got["n_cameras"] == 1 and got["start_camera"] == 0
        d = rc.dist(got["R"], got["tvec"], cam.R.T @ one["R"], cam.R.T @ (one["tvec"] - cam.t))
        worst = max(worst, d)
        assert d < 1e-6, (rig, len(entries), d)
        assert abs(got["image_error"] - one["image_error"]) < 1e-6 and got["err_per_camera"][0] == got["image_error"]
        _check_record(got)
    print("one-camera rig,", rig, ": largest distance to fid_map_pose's record", worst)
    det.set_map(None)
    det.set_rig(None)


# ------------------------------------------------------------------------------------------------ 2. and 3. the restatement, the minimum
@pytest.mark.parametrize("name", [c.name for c in rc.cases()])
def test_the_kernel_against_the_restatement_and_the_minimum(det, name):
    """R, tvec within 1e-6 of the restatement, the integer fields equal; exact projections give the pose back; on the noisy cases the
    device is within FACTOR x rig_cases.gap_to_minimum() of the exact minimum of the joint reprojection error.  MEASURED on the CPU,
    restatement to minimum: 3.7e-10 (the bound: 3.7e-9); on the device (MI355X), device to minimum: 3.7e-10 at most (two cameras with
    one marker each), 2.0e-10 with the middle camera blind, below 4e-11 on the other noisy cases; device to restatement: 2.8e-10 at most
    (one noisy marker in one camera), 2e-15 and below elsewhere."""
    c = rc.case(name)
    want = rc.restated(name)
    got = _run(det, c)
    _same_integers(got, want)
    d = rc.dist(got["R"], got["tvec"], want["R"], want["tvec"])
    print(name, "distance to the restatement", d)
    assert d < 1e-6, (name, d)
    assert abs(got["image_error"] - want["image_error"]) < 1e-9 + 1e-6 * want["image_error"]
    assert np.abs(got["err_per_camera"] - want["err_per_camera"]).max() < 1e-9 + 1e-6 * want["err_per_camera"].max()
    _check_record(got)
    if c.noisy:
        bound = FACTOR * rc.gap_to_minimum()
        pm = rr.exact_minimum(c.cams, want["pcam"], want["P"], want["img"], np.concatenate([rr.rotvec(c.R), c.t]))
        dm = rc.dist(got["R"], got["tvec"], rr.rodrigues(pm[:3]), pm[3:])
        print(name, "distance to the exact minimum", dm, "bound", bound)
        assert dm < bound, (name, dm, bound)
    else:
        # (float32 corners: the 4-point case is the least determined, 1.4e-6 on the CPU)
        assert rc.dist(got["R"], got["tvec"], c.R, c.t) < 1e-5
    if name.startswith("three_over"):
        assert got["n_markers"] == _lib.RIG_MAX_USED and got["n_over"] == 3


def test_nobody_sees_the_map(det):
    c = rc.case("two_cameras")
    det.set_map(c.entries)
    det.set_rig(rc.lib_rig(c.cams))
    got = det.rig_pose([c.corners[0][:2], c.corners[1][:1]], [[900, 901], [902]])
    assert got["n_markers"] == 0 and got.tobytes() == np.zeros(1, RIG_POSE_DTYPE).tobytes()
    assert det.rig_pose([np.zeros((0, 4, 2)), np.zeros((0, 4, 2))], [[], []]).tobytes() == got.tobytes()
    rec, cov = det.rig_pose([np.zeros((0, 4, 2)), np.zeros((0, 4, 2))], [[], []], sigma_px=1.0)
    assert rec.tobytes() == got.tobytes() and cov["pose"]["status"] == 1 and not cov["cov_cam_pose"].any()


def test_every_byte_of_a_record_is_written():
    """The record has no padding (reserved0 fills the gap in front of the doubles and is 0), so the byte comparisons of this file
    compare nothing the kernel did not write: a detector made after another one's blocks were freed gives the bytes the first gave."""
    assert sum(RIG_POSE_DTYPE.fields[n][0].itemsize for n in RIG_POSE_DTYPE.names) == RIG_POSE_DTYPE.itemsize
    c = rc.case("two_cameras_noisy")
    got = []
    for _ in range(2):
        d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=2, max_markers=32)
        try:
            got.append(_run(d, c))
        finally:
            d.close()
    assert got[0].tobytes() == got[1].tobytes() and got[0]["reserved0"] == 0


# ------------------------------------------------------------------------------------------------ 4. gather rules
def test_gather_rules(det):
    c = rc.case("two_cameras_noisy")
    det.set_map(c.entries)
    det.set_rig(rc.lib_rig(c.cams))
    base = det.rig_pose(c.corners, c.ids)
    assert base["n_markers"] == 10 and base["n_per_camera"][:2].tolist() == [6, 4]
    # an id twice in camera 0's frame is dropped from that frame only; camera 1 still uses it.  The same id in two cameras is used twice.
    ids0 = np.concatenate([c.ids[0], c.ids[0][:1], [999]])
    corners0 = np.concatenate([c.corners[0], c.corners[0][:1] + 40, c.corners[0][:1] + 80])
    assert int(c.ids[0][0]) in c.ids[1].tolist()
    got = det.rig_pose([corners0, c.corners[1]], [ids0, c.ids[1]])
    without = det.rig_pose([c.corners[0][1:], c.corners[1]], [c.ids[0][1:], c.ids[1]])
    assert got["n_markers"] == 9 and got["n_per_camera"][:2].tolist() == [5, 4] and got.tobytes() == without.tobytes()
    want = rr.restate(c.cams, c.entries, [ids0, c.ids[1]], [corners0, c.corners[1]])
    _same_integers(got, want)
    assert rc.dist(got["R"], got["tvec"], want["R"], want["tvec"]) < 1e-6


def test_an_equidistant_corner_past_89_degrees_costs_its_marker(det):
    c = rc.case("three_models_noisy")
    assert c.cams[1].model == rr.cm.EQUIDISTANT
    det.set_map(c.entries)
    det.set_rig(rc.lib_rig(c.cams))
    far = np.array([[[1120, 240], [1150, 240], [1150, 270], [1120, 270]]], np.float32)  # theta_d = 800 / 466.7 = 1.71 > theta_d(89 degrees) = 1.67
    assert not rr.undistort(c.cams[1].model, c.cams[1].K, c.cams[1].D, 1120.0, 240.0)[2]
    ids = [c.ids[0], c.ids[1].copy(), c.ids[2]]
    corners = [c.corners[0], c.corners[1].copy(), c.corners[2]]
    corners[1][2] = far[0]
    got = det.rig_pose(corners, ids)
    want = rr.restate(c.cams, c.entries, ids, corners)
    assert got["n_unposable"] == 1 and got["n_markers"] == 13 and got["n_per_camera"][:3].tolist() == [4, 5, 4]
    _same_integers(got, want)
    assert rc.dist(got["R"], got["tvec"], want["R"], want["tvec"]) < 1e-6
    # the same corners under a pinhole camera are just a bad observation: nothing is unposable there
    corners0 = [c.corners[0].copy(), c.corners[1], c.corners[2]]
    corners0[0][1] = far[0]
    assert det.rig_pose(corners0, ids)["n_unposable"] == 0


# ------------------------------------------------------------------------------------------------ 5. start camera
def test_the_start_camera(det):
    """The largest summed area wins: in every case the restatement's choice (above), and here a camera that is handed larger
    markers; of equals the lowest index: two identical cameras at mirrored extrinsics whose corner lists are mirror images, areas equal
    bit for bit, in either order of the cameras."""
    cams, e, ids, corners = rc.mirrored_tie()
    a = [sum(rr.shoelace(q) for q in cc_) for cc_ in corners]
    assert a[0] == a[1]
    det.set_map(e)
    det.set_rig(rc.lib_rig(cams))
    got = det.rig_pose(corners, ids)
    assert got["start_camera"] == 0 and got["n_per_camera"][:2].tolist() == [4, 4]
    want = rr.restate(cams, e, ids, corners)
    assert rc.dist(got["R"], got["tvec"], want["R"], want["tvec"]) < 1e-6
    det.set_rig(rc.lib_rig(cams[::-1]))
    swapped = det.rig_pose(corners[::-1], ids[::-1])
    assert swapped["start_camera"] == 0
    # camera 1 sees one marker less: camera 0 has the larger sum; camera 0 sees one less: camera 1 has
    det.set_rig(rc.lib_rig(cams))
    assert det.rig_pose([corners[0], corners[1][:3]], [ids[0], ids[1][:3]])["start_camera"] == 0
    assert det.rig_pose([corners[0][:3], corners[1]], [ids[0][:3], ids[1]])["start_camera"] == 1


# ------------------------------------------------------------------------------------------------ 6. and 7. determinism, batches, frames
def _scene_detector_inputs():
    frames = rc.scene_frames()
    return frames, np.stack([f.image for f in frames])


def test_rendered_frames_end_to_end_batches_and_determinism(det):
    """synth.make_rig_frames: two cameras 12 cm apart with converging axes, a 3 x 2 board.  Every id is found in both frames; the device
    pose is within 1e-6 of the restatement on the device's own corners; 3 time steps x 2 cameras through detect_markers_batch +
    rig_pose_last equal the three rig_pose calls on the per-frame results byte for byte, the same behind submit_batch / collect; the
    same call twice gives the same bytes; 5 frames with a 2-camera rig are refused."""
    frames, pair = _scene_detector_inputs()
    e = mc.scene_map("3x2")
    det.set_map(e)
    det.set_rig(rc.lib_rig(rc.SCENE_RIG))
    per_frame = det.detect_markers_batch(pair)
    for (corners, ids), f in zip(per_frame, frames):
        assert sorted(ids.tolist()) == sorted(f.ids.tolist())
    got = det.rig_pose_last()
    assert len(got) == 1 and got[0]["n_markers"] == 12 and got[0]["n_per_camera"][:2].tolist() == [6, 6]
    want = rr.restate(rc.SCENE_RIG, e, [ids for _, ids in per_frame], [corners for corners, _ in per_frame])
    d = rc.dist(got[0]["R"], got[0]["tvec"], want["R"], want["tvec"])
    R, t = rc.scene_pose()
    print("rendered rig frames: distance to the restatement on the device's corners", d, "; to the rendered truth", rc.dist(got[0]["R"], got[0]["tvec"], R, t),
          "; image_error", float(got[0]["image_error"]), "per camera", got[0]["err_per_camera"][:2].tolist())
    assert d < 1e-6
    assert det.rig_pose_last().tobytes() == got.tobytes()
    # three time steps: the pair, the pair with its cameras' frames darkened (other corners), the pair again
    dim = (pair.astype(np.float32) * 0.8 + 20).astype(np.uint8)
    six = np.concatenate([pair, dim, pair])
    res = det.detect_markers_batch(six)
    last, last_cov = det.rig_pose_last(sigma_px=0.5)
    assert len(last) == 3 and det.rig_pose_last().tobytes() == last.tobytes()
    for s in range(3):
        one, one_cov = det.rig_pose([res[2 * s][0], res[2 * s + 1][0]], [res[2 * s][1], res[2 * s + 1][1]], sigma_px=0.5)
        assert one.tobytes() == last[s].tobytes() and one_cov.tobytes() == last_cov[s].tobytes()
    assert last[0].tobytes() == got[0].tobytes() == last[2].tobytes()
    det.submit_batch(six)
    with pytest.raises(FidError):  # a batch in flight
        det.rig_pose_last()
    det.collect()
    assert det.rig_pose_last().tobytes() == last.tobytes()
    # 5 frames are no whole number of time steps of a 2-camera rig
    det.detect_markers_batch(six[:5])
    with pytest.raises(FidError) as ei:
        det.rig_pose_last()
    assert ei.value.status == _lib.FID_E_INVALID_ARG and "multiple" in str(ei.value)
    det.set_map(None)
    det.set_rig(None)


# ------------------------------------------------------------------------------------------------ 8. covariance
@pytest.mark.parametrize("sigma_px", [1.0, 0.0])
def test_covariance(det, sigma_px):
    """cov_rt = sigma^2 (J^T J)^-1 from the restatement's Jacobian at the RETURNED pose, to the relative bound test_gpu_pose_cov.py
    uses: the whitened deviation below pose_cov_cases.tol(), 100 x the disagreement of two float64 CPU inverses over that file's cases
    (5.11e-11); the three matrices symmetric bit for bit; cov == NULL gives the same pose bytes."""
    tol = cc.tol()
    for name in ["two_cameras_noisy", "three_models_noisy", "seventeen_noisy", "one_marker_one_camera_noisy"]:
        c = rc.case(name)
        got, cov = _run(det, c, sigma_px)
        assert _run(det, c).tobytes() == got.tobytes()
        want = rc.restated(name)
        ref = rr.covariance(c.cams, want["pcam"], want["P"], want["img"], np.concatenate([got["rvec"], got["tvec"]]), sigma_px)
        assert cov["pose"]["status"] == 0 and cov["pose"]["n_points"] == ref["n_points"]
        assert abs(cov["pose"]["sigma2"] - ref["sigma2"]) <= 1e-9 * ref["sigma2"]
        for key, m in (("cov_rt", cov["pose"]["cov_rt"]), ("cov_pose", cov["pose"]["cov_pose"]), ("cov_cam_pose", cov["cov_cam_pose"])):
            assert np.array_equal(m, m.T), (name, key)
            dev = cc.whitened_dev(m, ref[key])
            print(name, key, "whitened deviation", dev)
            assert dev < tol, (name, key, dev, tol)
    det.set_map(None)
    det.set_rig(None)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(det):
    L = _lib.load()
    c = rc.case("two_cameras_noisy")
    det.set_map(c.entries)
    det.set_rig(rc.lib_rig(c.cams))
    before = det.rig_pose(c.corners, c.ids)

    def still_answers():
        assert det.rig_pose(c.corners, c.ids).tobytes() == before.tobytes()

    def rc_of(cams):
        tab = (_lib.FidRigCamera * len(cams))(*[x.c for x in cams])
        return L.fid_set_rig(det._ctx, tab, len(cams))

    good = rc.lib_rig(c.cams)
    assert rc_of(good * 8) == _lib.FID_OK  # (16 cameras are a rig)
    det.set_rig(good)
    assert rc_of(good * 8 + good[:1]) == _lib.FID_E_UNSUPPORTED and b"16" in L.fid_last_error(det._ctx)
    still_answers()
    bad = rc.lib_rig(c.cams)
    bad[1].c.cam.model = 3
    assert rc_of(bad) == _lib.FID_E_INVALID_ARG and b"model" in L.fid_last_error(det._ctx)
    still_answers()
    skew = c.cams[1].R.copy()
    skew[0, 1] += 1e-8
    assert rc_of([good[0], RigCamera(Camera(c.cams[1].model, c.cams[1].K, c.cams[1].D), skew, c.cams[1].t)]) == _lib.FID_E_INVALID_ARG
    assert b"1e-9" in L.fid_last_error(det._ctx)
    still_answers()
    mirror = c.cams[1].R * np.array([[-1.0], [1.0], [1.0]])
    assert rc_of([good[0], RigCamera(Camera(c.cams[1].model, c.cams[1].K, c.cams[1].D), mirror, c.cams[1].t)]) == _lib.FID_E_INVALID_ARG
    still_answers()
    for field in ("K", "D", "R", "t"):
        nan = rc.lib_rig(c.cams)
        assert nan[0].c.cam.n_dist > 1
        (getattr(nan[0].c.cam, field) if field in ("K", "D") else getattr(nan[0].c, field))[1] = float("inf")
        assert rc_of(nan) == _lib.FID_E_INVALID_ARG and b"finite" in L.fid_last_error(det._ctx), field
        still_answers()
    # a batch in flight refuses fid_set_rig, fid_rig_pose and fid_rig_pose_last
    _, pair = _scene_detector_inputs()
    det.submit_batch(pair)
    assert rc_of(good) == _lib.FID_E_INVALID_ARG and b"in flight" in L.fid_last_error(det._ctx)
    with pytest.raises(FidError) as ei:
        det.rig_pose(c.corners, c.ids)
    assert ei.value.status == _lib.FID_E_INVALID_ARG and "in flight" in str(ei.value)
    with pytest.raises(FidError) as ei:
        det.rig_pose_last()
    assert ei.value.status == _lib.FID_E_INVALID_ARG and "in flight" in str(ei.value)
    det.collect()
    still_answers()
    # fid_rig_pose_last: room for too few time steps
    out = np.zeros(1, RIG_POSE_DTYPE)
    det.detect_markers_batch(np.concatenate([pair, pair]))
    assert L.fid_rig_pose_last(det._ctx, out.ctypes.data, 1, 0.0, None) == _lib.FID_E_CAPACITY
    cov = np.zeros(2, MAP_POSE_COV_DTYPE)
    out2 = np.zeros(2, RIG_POSE_DTYPE)
    for bad_sigma in (-1.0, float("nan")):
        assert L.fid_rig_pose_last(det._ctx, out2.ctypes.data, 2, bad_sigma, cov.ctypes.data) == _lib.FID_E_INVALID_ARG
    assert L.fid_rig_pose_last(det._ctx, out2.ctypes.data, 2, -1.0, None) == _lib.FID_OK  # (without cov sigma_px is not read)
    still_answers()
    # no rig, no map
    det.set_rig(None)
    with pytest.raises(FidError) as ei:
        det.rig_pose_last()
    assert "no rig" in str(ei.value)
    det.set_rig(good)
    det.set_map(None)
    with pytest.raises(FidError) as ei:
        det.rig_pose_last()
    assert "no map" in str(ei.value)
    det.set_map(c.entries)
    still_answers()
    det.set_map(None)
    det.set_rig(None)
