"""ChArUco boards on the device (include/fid_abi.h: "ChArUco boards"; fid_charuco.hip) against the NumPy restatement, stage by stage: the
kept corners and their order, the positions to 2 float ulps, the windows recomputed from the device's own positions, the refined corners
bit for bit against oracle.corner_subpix started where the device started; the pose against oracle.solve_pnp_points; the calls on the
last detect call against the calls that bring their input from the host, byte for byte."""
import ctypes as C
import functools

import numpy as np
import pytest

import aruco_map_cases as mc
import charuco_cases as cc
import charuco_restatement as cr
from fiducials_amd import _lib, synth
from fiducials_amd.camera import Camera
from fiducials_amd.detector import ArucoDetector, FidError

pytestmark = pytest.mark.gpu

Z5 = np.zeros(5)
FACTOR = 10.0  # (tests/test_gpu_aruco_map.py: ten times the oracle's own gap to the exact minimum)


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(cc.DICT, max_width=cc.W, max_height=cc.H, max_batch=4, max_markers=64)
    yield d
    d.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_stages(det, bname, ids, corners, image, min_markers, cam_positions=None, **cam):
    """One charuco_interpolate call held to the restatement; returns the records."""
    b = cc.rboard(bname)
    got = det.charuco_interpolate(corners, ids, image, min_markers=min_markers, **cam)
    kept, pos, _ = cr.interpolate(b, ids, corners, cc.W, cc.H, min_markers, cam_positions)
    assert got["id"].tolist() == kept.tolist(), (bname, min_markers)
    if len(kept):
        u = max(cc.ulps(got["x0"], pos[:, 0]).max(), cc.ulps(got["y0"], pos[:, 1]).max())
        print(bname, "min_markers", min_markers, "corners", len(kept), "positions: worst", u, "ulps; windows", got["win"].min(), "..", got["win"].max())
        assert u <= 2.0, (bname, u)
    assert got["win"].tolist() == cr.device_windows(b, ids, corners, got).tolist()
    want = cr.refine(image, np.stack([got["x0"], got["y0"]], axis=1), got["win"])
    assert np.array_equal(_bits(want[:, 0]), _bits(got["x"])) and np.array_equal(_bits(want[:, 1]), _bits(got["y"])), (bname, min_markers)
    return got


# ------------------------------------------------------------------------------------------------ the kernels on hand-made markers
def test_the_whole_board_near_middle_and_far(det):
    """The 5 x 4 board whole, at three distances: windows of 10 (near), of 4 .. 7 (middle), clamped to 1 (far)."""
    det.set_charuco_board(cc.board("5x4"))
    for name, tilt, dist, lo, hi in (("near", (0.1, -0.1, 0.0), 0.36, 10, 10), ("middle", (0.3, -0.2, 0.0), 0.72, 4, 7), ("far", (0.2, 0.1, 0.0), 1.8, 1, 1)):
        R, t = cc.board_pose("5x4", tilt, dist, roll=0.3)
        fr = synth.make_charuco_frame(cc.dictionary(), cc.board("5x4"), cc.K, R, t, seed=3, width=cc.W, height=cc.H)
        ids, corners = cc.hand_markers("5x4", R, t, seed=21)
        for mm in (2, 1):
            got = _check_stages(det, "5x4", ids, corners, fr.image, mm)
            assert len(got) == 12 and lo <= got["win"].min() and got["win"].max() <= hi, (name, got["win"])
        if name == "near":
            assert np.abs(np.stack([got["x"], got["y"]], axis=1) - fr.corners_image).max() < 0.5  # (the refined corners are the picture's)
    det.set_charuco_board(None)


@functools.lru_cache(maxsize=None)
def _near_case():
    R, t = cc.board_pose("5x4", (0.25, 0.2, 0.0), 0.40, roll=-0.2)
    fr = synth.make_charuco_frame(cc.dictionary(), cc.board("5x4"), cc.K, R, t, seed=5, width=cc.W, height=cc.H)
    fr.image.setflags(write=False)
    return R, t, fr


def test_removed_duplicated_and_foreign_markers(det):
    """Markers removed so that corners have 2, 1 and 0 detected neighbours; an id listed twice is left out altogether; a marker of another
    board is passed over; first_id other than 0."""
    R, t, fr = _near_case()
    det.set_charuco_board(cc.board("5x4"))
    b = cc.rboard("5x4")
    keep = [0, 1, 3, 4, 6, 9]  # (markers 2, 5, 7, 8 lost)
    ids, corners = cc.hand_markers("5x4", R, t, seed=22, keep=keep)
    ndet = [sum(int(k) in keep for k in b.near_marker[i]) for i in range(b.n_corners)]
    assert {0, 1, 2} <= set(ndet)
    got2 = _check_stages(det, "5x4", ids, corners, fr.image, 2)
    got1 = _check_stages(det, "5x4", ids, corners, fr.image, 1)
    assert got2["id"].tolist() == [i for i in range(12) if ndet[i] == 2] and got1["id"].tolist() == [i for i in range(12) if ndet[i] >= 1]
    # marker 4 listed twice (the second time somewhere else), and markers 200, 201 of another board in between
    ids_all, corners_all = cc.hand_markers("5x4", R, t, seed=23)
    ids_d = np.concatenate([ids_all[:5], [200], ids_all[5:], [4, 201]]).astype(np.int32)
    corners_d = np.concatenate([corners_all[:5], corners_all[:1] + 7, corners_all[5:], corners_all[4:5] + 30, corners_all[1:2] - 9])
    got = _check_stages(det, "5x4", ids_d, corners_d, fr.image, 1)
    without4 = _check_stages(det, "5x4", np.delete(ids_all, 4), np.delete(corners_all, 4, axis=0), fr.image, 1)
    assert got.tobytes() == without4.tobytes() and len(got) == 12
    # the same board with ids 40 .. 49; the ids 0 .. 9 now belong to another board
    det.set_charuco_board(cc.board("5x4_id40"))
    ids40, corners40 = cc.hand_markers("5x4_id40", R, t, seed=23)
    assert ids40.tolist() == list(range(40, 50)) and np.array_equal(corners40, corners_all)
    got40 = _check_stages(det, "5x4_id40", ids40, corners40, fr.image, 2)
    assert got40.tobytes() == _check_stages(det, "5x4_id40", np.concatenate([ids_all, ids40]), np.concatenate([corners_all + 3, corners40]), fr.image, 2).tobytes()
    assert len(det.charuco_interpolate(corners_all, ids_all, fr.image)) == 0
    det.set_charuco_board(None)


def test_corners_at_the_edge_of_the_frame(det):
    """The board moved so that its first column of corners falls within 2 px of the frame's left edge (dropped) and the next ones land
    where the window leaves the frame (refined through the replicated border)."""
    det.set_charuco_board(cc.board("5x4"))
    b = cc.board("5x4")
    R, t = cc.board_pose("5x4", (0.0, 0.0, 0.0), 0.40)
    u0 = cc.project(b.corner_object_points[:1], R, t, cc.K, Z5)[0, 0]
    t = t - np.array([(u0 - 1.2) * 0.40 / cc.K[0, 0], 0.0, 0.0])  # corner 0 to x = 1.2
    fr = synth.make_charuco_frame(cc.dictionary(), b, cc.K, R, t, seed=6, width=cc.W, height=cc.H)
    ids, corners = cc.hand_markers("5x4", R, t, seed=24)
    got = _check_stages(det, "5x4", ids, corners, fr.image, 1)
    assert got["id"].tolist() == [i for i in range(12) if i % 4 != 0] and got["x0"].min() < 60
    # ... and a corner at the top edge
    R, t = cc.board_pose("5x4", (0.0, 0.0, 0.0), 0.40)
    v0 = cc.project(b.corner_object_points[8:9], R, t, cc.K, Z5)[0, 1]
    t = t - np.array([0.0, (v0 - 4.5) * 0.40 / cc.K[1, 1], 0.0])  # the top row of corners to y = 4.5: kept, the window leaves the frame
    fr = synth.make_charuco_frame(cc.dictionary(), b, cc.K, R, t, seed=7, width=cc.W, height=cc.H)
    ids, corners = cc.hand_markers("5x4", R, t, seed=25)
    got = _check_stages(det, "5x4", ids, corners, fr.image, 1)
    assert len(got) == 12 and got["y0"].min() < 6
    det.set_charuco_board(None)


@functools.lru_cache(maxsize=None)
def _case_10x9():
    R, t = cc.board_pose("10x9", (0.2, -0.15, 0.0), 0.36, roll=0.1)
    fr = synth.make_charuco_frame(cc.dictionary(), cc.board("10x9"), cc.K, R, t, seed=8, width=cc.W, height=cc.H)
    fr.image.setflags(write=False)
    return R, t, fr


def test_more_corners_than_lanes(det):
    """10 x 9: 72 corners and 45 markers, more than one pass of 64 lanes; some markers lost."""
    R, t, fr = _case_10x9()
    det.set_charuco_board(cc.board("10x9"))
    ids, corners = cc.hand_markers("10x9", R, t, seed=26)
    assert len(_check_stages(det, "10x9", ids, corners, fr.image, 2)) == 72
    keep = [k for k in range(45) if k % 7 != 3]
    ids, corners = cc.hand_markers("10x9", R, t, seed=27, keep=keep[::-1])  # (list order is not marker order)
    got = _check_stages(det, "10x9", ids, corners, fr.image, 2)
    assert 40 < len(got) < 72 and len(_check_stages(det, "10x9", ids, corners, fr.image, 1)) == 72
    det.set_charuco_board(None)


def test_the_largest_board_on_a_flat_image(det):
    """22 x 23: 253 markers (FID_MAP_MAX_USED is 256), 462 corners, on a flat gray image: the refinement leaves the start where it is."""
    big = ArucoDetector(cc.DICT, max_width=cc.W, max_height=cc.H, max_markers=256)
    try:
        big.set_charuco_board(cc.board("22x23"))
        R, t = cc.board_pose("22x23", (0.05, -0.05, 0.0), 0.74)
        ids, corners = cc.hand_markers("22x23", R, t, seed=28)
        assert len(ids) == 253
        got = _check_stages(big, "22x23", ids, corners, cc.flat_gray(), 2)
        assert len(got) > 400 and np.array_equal(got["x"], got["x0"]) and np.array_equal(got["y"], got["y0"])
        cam = _check_stages(big, "22x23", ids, corners, cc.flat_gray(), 2, cam_positions=_cam_positions(big, "22x23", ids, corners, Z5), K=cc.K, D=Z5)
        assert len(cam) > 400
    finally:
        big.close()


# ------------------------------------------------------------------------------------------------ the camera route
def _cam_positions(det, bname, ids, corners, Dv):
    """every chessboard corner projected under the record fid_map_pose_cam returns with the board's markers as the map"""
    b = cc.board(bname)
    det.set_map(b.as_map_entries())
    rec = det.map_pose(cc.K, Dv, corners, ids)
    det.set_map(None)
    assert rec["n_markers"] > 0
    return det.project_points(Camera(_lib.CAM_PLUMB_BOB, cc.K, Dv), rec["rvec"], rec["tvec"], b.corner_object_points)


def test_the_camera_route_projects_under_the_map_pose(det):
    R, t, fr = _near_case()
    det.set_charuco_board(cc.board("5x4_dyadic"))
    Rd, td = cc.board_pose("5x4_dyadic", (0.25, 0.2, 0.0), 0.32, roll=-0.2)
    for keep in (None, [0, 2, 3, 5, 8]):
        ids, corners = cc.hand_markers("5x4_dyadic", Rd, td, seed=29, D=mc.D_NONZERO, keep=keep)
        uv = _cam_positions(det, "5x4_dyadic", ids, corners, mc.D_NONZERO)
        for mm in (2, 1):
            got = _check_stages(det, "5x4_dyadic", ids, corners, fr.image, mm, cam_positions=uv, K=cc.K, D=mc.D_NONZERO)
            assert len(got) >= 4
    # the other two models: the rational one with its extra terms zero is the plumb-bob one bit for bit; the fisheye one runs
    ids, corners = cc.hand_markers("5x4_dyadic", Rd, td, seed=29, D=mc.D_NONZERO)
    pb = det.charuco_interpolate(corners, ids, fr.image, K=cc.K, D=mc.D_NONZERO)
    rat = det.charuco_interpolate(corners, ids, fr.image, camera=Camera(_lib.CAM_RATIONAL, cc.K, np.concatenate([mc.D_NONZERO, np.zeros(3)])))
    assert rat.tobytes() == pb.tobytes()
    fe = det.charuco_interpolate(corners, ids, fr.image, camera=Camera(_lib.CAM_EQUIDISTANT, cc.K, [0.0, 0.0, 0.0, 0.0]))
    assert fe["id"].tolist() == pb["id"].tolist() and np.isfinite(fe["x"]).all() and np.isfinite(fe["y"]).all()
    # no board marker in the list: no pose, no corners
    assert len(det.charuco_interpolate(corners + 1, ids + 500, fr.image, K=cc.K, D=mc.D_NONZERO)) == 0
    det.set_charuco_board(None)


def test_on_a_distorted_picture_the_camera_route_is_nearer_the_truth(det):
    fr = cc.view("frontal", distorted=True)
    Dv = mc.D_NONZERO * 4
    det.set_charuco_board(cc.board("5x4"))
    corners, ids = det.detect_markers(fr.image)
    assert len(ids) >= 9
    hom, cam = det.charuco_last()[0], det.charuco_last(K=cc.K, D=Dv)[0]
    assert hom["id"].tolist() == cam["id"].tolist() and len(hom) >= 10
    truth = fr.corners_image[hom["id"]]
    eh = np.linalg.norm(np.stack([hom["x0"], hom["y0"]], axis=1) - truth, axis=1)
    ec = np.linalg.norm(np.stack([cam["x0"], cam["y0"]], axis=1) - truth, axis=1)
    print("distorted picture: mean distance of the positions to the truth, homographies %.3f px, camera %.3f px" % (eh.mean(), ec.mean()))
    assert ec.mean() < eh.mean()
    det.set_charuco_board(None)


# ------------------------------------------------------------------------------------------------ the pose
def _check_pose_record(got):
    assert np.abs(got["R"] - synth._rodrigues(got["rvec"])).max() < 1e-12
    assert np.abs(got["cam_R"] - got["R"].T).max() < 1e-12 and np.abs(got["cam_t"] + got["R"].T @ got["tvec"]).max() < 1e-12


def test_the_pose_matches_the_oracle(det):
    """At most 32 corners: R and tvec to 1e-6 against cv::solvePnP restated on the same points; image_error recomputed to 1e-9."""
    R, t, fr = _near_case()
    b = cc.rboard("5x4")
    det.set_charuco_board(cc.board("5x4"))
    for Dv in (Z5, mc.D_NONZERO):
        for keep in (None, [0, 1, 3, 4, 6, 9]):
            ids, corners = cc.hand_markers("5x4", R, t, seed=30, D=Dv, keep=keep)
            rec = det.charuco_interpolate(corners, ids, fr.image, min_markers=1)
            xy = np.stack([rec["x"], rec["y"]], axis=1)
            got = det.charuco_pose(xy, rec["id"], cc.K, Dv)
            assert got["status"] == _lib.CHARUCO_POSE_OK and got["n_corners"] == len(rec) <= 32
            r, tv = cr.pose(b, cc.K, Dv, rec["id"], xy)
            d = max(np.abs(got["R"] - synth._rodrigues(r)).max(), np.abs(got["tvec"] - tv).max())
            print("pose over", len(rec), "corners: distance to the oracle", d)
            assert d < 1e-6
            _check_pose_record(got)
            dd = xy.astype(np.float64) - cc.project(b.corner_obj[rec["id"]], got["R"], got["tvec"], cc.K, Dv).astype(np.float32).astype(np.float64)
            assert abs(got["image_error"] - float((dd * dd).sum() / len(rec))) < 1e-9
            assert np.abs(got["R"] - R).max() < 0.05 and np.abs(got["tvec"] - t).max() < 0.02  # (the picture's pose, roughly)
            assert det.charuco_pose(xy, rec["id"], cc.K, Dv).tobytes() == got.tobytes()
    det.set_charuco_board(None)


def test_the_pose_over_72_corners_is_at_the_minimum(det):
    R, t, fr = _case_10x9()
    b = cc.rboard("10x9")
    det.set_charuco_board(cc.board("10x9"))
    bound = FACTOR * mc.oracle_gap_to_minimum()
    Dv = mc.D_NONZERO
    rng = np.random.default_rng(31)
    xy = (cc.project(b.corner_obj, R, t, cc.K, Dv) + rng.uniform(-cc.NOISE_PX, cc.NOISE_PX, (72, 2))).astype(np.float32)
    got = det.charuco_pose(xy, np.arange(72), cc.K, Dv)
    assert got["status"] == _lib.CHARUCO_POSE_OK and got["n_corners"] == 72
    Rm, tm = cc.exact_minimiser(b.corner_obj, xy.astype(np.float64), R, t, cc.K, Dv)
    d = max(np.abs(got["R"] - Rm).max(), np.abs(got["tvec"] - tm).max())
    print("72 corners: distance to the exact minimum", d, "bound", bound)
    assert d < bound
    dd = xy.astype(np.float64) - cc.project(b.corner_obj, got["R"], got["tvec"], cc.K, Dv).astype(np.float32).astype(np.float64)
    assert abs(got["image_error"] - float((dd * dd).sum() / 72)) < 1e-9
    _check_pose_record(got)
    det.set_charuco_board(None)


def test_no_pose_from_too_few_corners_or_from_one_line(det):
    R, t, _ = _near_case()
    b = cc.rboard("5x4")
    det.set_charuco_board(cc.board("5x4"))
    uv = cc.project(b.corner_obj, R, t, cc.K, Z5).astype(np.float32)
    for ids, status in (([0, 5, 10], _lib.CHARUCO_POSE_FEW), ([], _lib.CHARUCO_POSE_FEW), ([0, 1, 2, 3], _lib.CHARUCO_POSE_COLLINEAR),
                        ([1, 5, 9, 9], _lib.CHARUCO_POSE_COLLINEAR), ([3, 6, 9, 6], _lib.CHARUCO_POSE_COLLINEAR), ([0, 1, 2, 7], _lib.CHARUCO_POSE_OK)):
        got = det.charuco_pose(uv[ids].reshape(-1, 2), ids, cc.K, Z5)
        assert got["status"] == status == cr.pose_status(b, ids) and got["n_corners"] == len(ids), (ids, got)
        if status != _lib.CHARUCO_POSE_OK:
            assert not got["rvec"].any() and not got["tvec"].any() and not got["R"].any() and not got["cam_R"].any() and got["image_error"] == 0
        else:
            assert np.abs(got["R"] - R).max() < 1e-3 and np.abs(got["tvec"] - t).max() < 1e-3
    with pytest.raises(FidError):
        det.charuco_pose(uv[:4], [0, 1, 2, 12], cc.K, Z5)  # (the board has corners 0 .. 11)
    det.set_charuco_board(None)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _batch_frames():
    frames = np.stack([cc.view("frontal").image, cc.view("tilted", hidden=(3,)).image, cc.view("far", hidden=(0, 7)).image,
                       cc.view("side", hidden=(5,)).image])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _single_frame_results():
    """per frame: (corners, ids, charuco_last without a camera, with one, charuco_pose_last), each from a single-frame call"""
    d = ArucoDetector(cc.DICT, max_width=cc.W, max_height=cc.H, max_batch=4, max_markers=64)
    try:
        d.set_charuco_board(cc.board("5x4"))
        out = []
        for img in _batch_frames():
            corners, ids = d.detect_markers(img)
            out.append((corners, ids, d.charuco_last()[0], d.charuco_last(K=cc.K, D=mc.D_NONZERO)[0], d.charuco_pose_last(cc.K, mc.D_NONZERO)[0].copy()))
        return out
    finally:
        d.close()


def test_the_last_call_equals_the_call_from_the_host(det):
    want = _single_frame_results()
    det.set_charuco_board(cc.board("5x4"))
    found = []
    for img, (corners, ids, hom, cam, pose) in zip(_batch_frames(), want):
        found.append(len(cr.gather(cc.rboard("5x4"), ids)))
        assert det.charuco_interpolate(corners, ids, img).tobytes() == hom.tobytes()
        assert det.charuco_interpolate(corners, ids, img, K=cc.K, D=mc.D_NONZERO).tobytes() == cam.tobytes()
        assert pose["n_corners"] == len(cam)
        if len(cam) >= 4:
            assert det.charuco_pose(np.stack([cam["x"], cam["y"]], axis=1), cam["id"], cc.K, mc.D_NONZERO).tobytes() == pose.tobytes()
            assert pose["status"] == _lib.CHARUCO_POSE_OK
        _check_stages(det, "5x4", ids, corners, img, 2)
    print("markers found per view", found, "corners", [len(w[2]) for w in want])
    assert found[0] == 10 and len(want[0][2]) == 12 and len(set(found)) > 1 and min(len(w[2]) for w in want) >= 4
    det.set_charuco_board(None)


def test_a_batch_equals_the_single_frame_calls(det):
    want = _single_frame_results()
    det.set_charuco_board(cc.board("5x4"))
    frames = np.ascontiguousarray(_batch_frames())
    for how in ("batch", "submit"):
        if how == "batch":
            res = det.detect_markers_batch(frames)
        else:
            det.submit_batch(frames)
            with pytest.raises(FidError) as e:
                det.charuco_last()  # a batch is in flight
            assert e.value.status == _lib.FID_E_INVALID_ARG and "in flight" in str(e.value)
            with pytest.raises(FidError):
                det.set_charuco_board(cc.board("5x4_id40"))
            res = det.collect()
        hom, cam, poses = det.charuco_last(), det.charuco_last(K=cc.K, D=mc.D_NONZERO), det.charuco_pose_last(cc.K, mc.D_NONZERO)
        assert len(hom) == len(cam) == len(poses) == 4
        for f in range(4):
            assert np.array_equal(res[f][0], want[f][0]) and np.array_equal(res[f][1], want[f][1])
            assert hom[f].tobytes() == want[f][2].tobytes() and cam[f].tobytes() == want[f][3].tobytes(), (how, f)
            assert poses[f].tobytes() == want[f][4].tobytes(), (how, f)
    det.set_charuco_board(None)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(det):
    L, ctx = det._L, det._ctx
    R, t, fr = _near_case()
    ids, corners = cc.hand_markers("5x4", R, t, seed=32)

    def set_board(*fields):
        b = _lib.FidCharucoBoard(*fields, 0)
        return L.fid_set_charuco_board(ctx, C.byref(b)), (L.fid_last_error(ctx) or b"").decode()

    det.set_charuco_board(None)
    with pytest.raises(FidError) as e:
        det.charuco_interpolate(corners, ids, fr.image)
    assert e.value.status == _lib.FID_E_INVALID_ARG and "no ChArUco board" in str(e.value)
    det.detect_markers(fr.image)
    with pytest.raises(FidError):
        det.charuco_last()
    with pytest.raises(FidError):
        det.charuco_pose_last(cc.K, Z5)
    for fields, status, word in (((1, 4, 0.04, 0.024, 0), _lib.FID_E_INVALID_ARG, "at least 2"), ((4, 1, 0.04, 0.024, 0), _lib.FID_E_INVALID_ARG, "at least 2"),
                                 ((23, 23, 0.04, 0.024, 0), _lib.FID_E_UNSUPPORTED, "512"), ((32, 17, 0.04, 0.024, 0), _lib.FID_E_UNSUPPORTED, "512"),
                                 ((5, 4, 0.04, 0.0, 0), _lib.FID_E_INVALID_ARG, "marker_len"), ((5, 4, 0.04, 0.04, 0), _lib.FID_E_INVALID_ARG, "marker_len"),
                                 ((5, 4, 0.04, 0.05, 0), _lib.FID_E_INVALID_ARG, "marker_len"), ((5, 4, 0.04, float("nan"), 0), _lib.FID_E_INVALID_ARG, "marker_len"),
                                 ((5, 4, float("inf"), 0.024, 0), _lib.FID_E_INVALID_ARG, "marker_len"),
                                 ((5, 4, 0.04, 0.024, 991), _lib.FID_E_INVALID_ARG, "dictionary"), ((5, 4, 0.04, 0.024, -1), _lib.FID_E_INVALID_ARG, "dictionary")):
        rc, text = set_board(*fields)
        assert rc == status and word in text, (fields, rc, text)
    assert set_board(32, 16, 0.04, 0.024, 0)[0] == _lib.FID_OK and set_board(5, 4, 0.04, 0.024, 990)[0] == _lib.FID_OK  # (the bounds themselves)
    det.set_charuco_board(cc.board("5x4"))
    rc, _ = set_board(1, 4, 0.04, 0.024, 0)  # a refused board leaves the one that is set
    assert rc == _lib.FID_E_INVALID_ARG and len(det.charuco_interpolate(corners, ids, fr.image)) == 12
    for mm in (0, 3, -1):
        with pytest.raises(FidError) as e:
            det.charuco_interpolate(corners, ids, fr.image, min_markers=mm)
        assert e.value.status == _lib.FID_E_INVALID_ARG and "min_markers" in str(e.value)
        with pytest.raises(FidError):
            det.charuco_last(min_markers=mm)
    with pytest.raises(FidError) as e:
        det.charuco_interpolate(corners, ids, fr.image, cap=5)
    assert e.value.status == _lib.FID_E_CAPACITY and det.last_charuco_counts.value == 12
    n_last = len(det.charuco_last()[0])
    assert n_last > 3
    with pytest.raises(FidError) as e:
        det.charuco_last(cap=3)
    assert e.value.status == _lib.FID_E_CAPACITY and det.last_charuco_counts.tolist() == [n_last]
    with pytest.raises(FidError):
        det.charuco_pose_last(cc.K, Z5, min_markers=0)
    det.set_charuco_board(None)


def test_a_detector_without_a_board_is_as_before(det):
    """Markers and fid_last_launches the same without a board, with one, after the ChArUco calls, and with it cleared again."""
    frames = np.ascontiguousarray(_batch_frames())

    def run():
        res = det.detect_markers_batch(frames)
        return b"".join(r[0].tobytes() + r[1].tobytes() for r in res), det.last_launches()

    det.set_charuco_board(None)
    plain = run()
    det.set_charuco_board(cc.board("5x4"))
    with_board = run()
    det.charuco_last()
    det.charuco_pose_last(cc.K, Z5)
    assert det.last_launches() == plain[1]
    after = run()
    det.set_charuco_board(None)
    assert plain == with_board == after == run()
