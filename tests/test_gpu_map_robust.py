"""The consensus map pose on the device (k_map_pose_robust, fid_map_pose_robust_cam, fid_map_pose_robust_last_cam) against its NumPy
restatement (tests/map_robust_restatement.py) on the planted cases of tests/map_robust_cases.py, and against the plain map pose
where the two must agree: the returned record is BYTE for byte what fid_map_pose_cam returns for the inlier markers in list order.

Every positive case asserts: the inlier set equals the restatement's, which equals the planted one; hypothesis, rounds and stable
are the restatement's; the pose bytes; worst_inlier_px <= inlier_px < best_outlier_px, both within 1e-9 of NumPy's err at the
returned pose.  A 640 x 480 context with max_batch = 4; most tests use no image."""
import functools

import numpy as np
import pytest

import aruco_map_cases as mc
import camera_model_cases as cm
import map_robust_cases as rc
import map_robust_restatement as rr
from fiducials_amd import _lib
from fiducials_amd.camera import Camera
from fiducials_amd.detector import (MAP_POSE_DTYPE, MAP_ROBUST_DTYPE, ArucoDetector, FidError, map_robust_outlier_ids,
                                    map_robust_outlier_positions)

pytestmark = pytest.mark.gpu

PX = rc.INLIER_PX


def _new_det():
    return ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=4, max_markers=32)


@pytest.fixture(scope="module")
def det():
    d = _new_det()
    yield d
    d.close()


def _camera(c: rc.Case) -> Camera:
    return Camera(c.model, mc.K, c.D)


def _run(det, c: rc.Case):
    det.set_map(c.entries)
    return det.map_pose_robust(camera=_camera(c), corners=c.corners, ids=c.ids, inlier_px=c.inlier_px, min_markers=c.min_markers)


def _zero_pose(pose):
    return pose.tobytes() == np.zeros(1, MAP_POSE_DTYPE)[0].tobytes()


def _check_positive(det, c: rc.Case, pose, rob):
    r = rc.restated(c.name)
    used = r["used"]
    assert rob["status"] == _lib.MAP_ROBUST_OK and rob["n_used"] == len(used)
    out_pos = map_robust_outlier_positions(rob).tolist()
    inl_pos = [k for k in range(len(used)) if k not in out_pos]
    assert inl_pos == r["inliers"], (c.name, inl_pos, r["inliers"])
    inl_list = [used[k] for k in inl_pos]
    assert tuple(inl_list) == c.planted
    assert rob["n_inliers"] == len(inl_pos) == pose["n_markers"] and rob["n_outliers"] == len(out_pos) and pose["n_over"] == r["n_over"]
    assert rob["hypothesis"] == r["hypothesis"], (c.name, rob["hypothesis"], r["hypothesis"])
    assert (rob["rounds"], rob["stable"]) == (r["rounds"], r["stable"]), (c.name, rob["rounds"], rob["stable"], r["rounds"], r["stable"])
    assert abs(rob["score"] - r["score"]) <= 1e-6 * r["score"], (c.name, rob["score"], r["score"])
    want_idx = [used[k] for k in out_pos][:16]
    assert rob["outlier_index"].tolist() == want_idx + [-1] * (16 - len(want_idx))
    assert map_robust_outlier_ids(rob, c.ids, c.entries["id"]).tolist() == [int(c.ids[used[k]]) for k in out_pos]
    # the pose: the plain call's bytes on the inlier markers in list order (n_over is the whole list's)
    plain = det.map_pose(camera=_camera(c), corners=c.corners[inl_list], ids=c.ids[inl_list]).copy()
    assert plain["n_over"] == 0
    plain["n_over"] = pose["n_over"]
    assert pose.tobytes() == plain.tobytes(), (c.name, "distance", np.abs(pose["R"] - plain["R"]).max(), np.abs(pose["tvec"] - plain["tvec"]).max())
    # the two margins under the returned pose, against NumPy's err
    by_id = {int(e["id"]): e for e in c.entries}
    errs = {}
    for k in r["eligible"]:
        e = by_id[int(c.ids[used[k]])]
        obj = rr.fid_corners(e["len"]) @ e["R"].T + e["t"]
        errs[k] = rr.err(c.model, mc.K, c.D, pose["R"], pose["tvec"], obj, c.corners[used[k]].astype(np.float64))
    worst = max(errs[k] for k in inl_pos)
    outs = [errs[k] for k in out_pos if k in errs]
    print(c.name, "worst inlier", rob["worst_inlier_px"], "best outlier", rob["best_outlier_px"], "score", rob["score"], "rounds", rob["rounds"])
    assert abs(rob["worst_inlier_px"] - worst) < 1e-9 and rob["worst_inlier_px"] <= c.inlier_px
    if outs:
        assert abs(rob["best_outlier_px"] - min(outs)) < 1e-9 and c.inlier_px < rob["best_outlier_px"]
    else:
        assert rob["best_outlier_px"] == -1.0


def _check_no_consensus(pose, rob, n_used):
    assert rob["status"] == _lib.MAP_ROBUST_NO_CONSENSUS and _zero_pose(pose)
    assert rob["n_used"] == n_used and rob["n_inliers"] == 0 and rob["n_outliers"] == n_used
    assert rob["worst_inlier_px"] == -1.0 and rob["best_outlier_px"] == -1.0
    assert map_robust_outlier_positions(rob).tolist() == list(range(n_used))


POSITIVE = [n for n, c in rc.cases().items() if c.planted is not None]


@pytest.mark.parametrize("name", POSITIVE)
def test_planted_case(det, name):
    """n = 1 .. 257, coplanar and not, three camera models, list bookkeeping, > 16 outliers, re-admission, four solves."""
    c = rc.cases()[name]
    pose, rob = _run(det, c)
    _check_positive(det, c, pose, rob)
    det.set_map(None)


def test_one_marker(det):
    """min_markers = 1: the plain pose bytes of that marker; min_markers = 2: no consensus and the zero record."""
    c = rc.cases()["n1_min1"]
    pose, rob = _run(det, c)
    assert pose.tobytes() == det.map_pose(camera=_camera(c), corners=c.corners, ids=c.ids).tobytes() and rob["hypothesis"] == 0
    c2 = rc.cases()["n1_min2"]
    pose, rob = _run(det, c2)
    _check_no_consensus(pose, rob, 1)
    assert rob["hypothesis"] == 0 and rob["rounds"] == 0
    det.set_map(None)


def test_two_markers_that_disagree(det):
    c = rc.cases()["n2_disagree"]
    assert rc.restated(c.name)["status"] == rr.NO_CONSENSUS
    pose, rob = _run(det, c)
    _check_no_consensus(pose, rob, 2)
    assert rob["outlier_index"].tolist() == [0, 1] + [-1] * 14
    det.set_map(None)


def test_the_largest_marker_can_be_the_outlier():
    """Among the n = 3 cases the outlier is, in one of them, the marker of largest image area (the plain kernel's non-coplanar
    start, and the first hypothesis by rank)."""
    hit = 0
    for bad in range(3):
        c = rc.cases()[f"n3_bad{bad}"]
        areas = [rc._area(q.astype(np.float64)) for q in c.corners]
        hit += int(np.argmax(areas)) == bad
    assert hit >= 1


def test_the_consensus_follows_five_moved_together(det):
    """Documented: more than half of the markers moved rigidly -- the pose is relative to them."""
    c = rc.cases()["floor8_5moved"]
    assert c.planted == (0, 2, 3, 5, 7)
    pose, rob = _run(det, c)
    assert map_robust_outlier_positions(rob).tolist() == [1, 4, 6]
    det.set_map(None)


def test_a_marker_past_89_degrees_is_flagged_not_fatal(det):
    c = rc.cases()["fisheye_past89"]
    det.set_map(c.entries)
    plain = det.map_pose(camera=_camera(c), corners=c.corners, ids=c.ids)
    assert plain["image_error"] == -1.0 and not plain["R"].any()  # the plain call voids the frame
    pose, rob = _run(det, c)
    assert map_robust_outlier_positions(rob).tolist() == [3] and rob["best_outlier_px"] == -1.0 and pose["n_markers"] == 7
    det.set_map(None)


def test_more_than_sixteen_outliers_leave_the_mask_complete(det):
    c = rc.cases()["grid40_18bad"]
    pose, rob = _run(det, c)
    pos = map_robust_outlier_positions(rob).tolist()
    assert pos == list(range(1, 37, 2)) and rob["n_outliers"] == 18 and rob["outlier_index"].tolist() == pos[:16]
    det.set_map(None)


# ------------------------------------------------------------------------------------------------ batches, on the markers where they lie
@functools.lru_cache(maxsize=None)
def _lying_map():
    """The 3 x 2 board's map with entry 25 moved, and the 2 x 2 board's with 11, 12 and 13 moved apart (no two markers of it agree)."""
    a, b = mc.scene_map("3x2").copy(), mc.scene_map("2x2").copy()
    a["t"][5] += [0.05, 0.04, 0.0]
    b["t"][1] += [0.06, 0.0, 0.0]
    b["t"][2] += [-0.05, 0.05, 0.0]
    b["t"][3] += [0.0, -0.07, 0.03]
    e = np.concatenate([a, b])
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _batch_frames():
    """Four outcomes: all inliers (the 3 x 2 board without its marker 25), one outlier (all six), no consensus (the 2 x 2 board),
    no markers (a blank frame)."""
    frames = np.stack([mc.scene("3x2", 1, without=5).image, mc.scene("3x2", 1).image, mc.scene("2x2", 1).image, np.full((mc.H, mc.W), 200, np.uint8)])
    frames.setflags(write=False)
    return frames


CAM_D = Camera(cm.PLUMB_BOB, mc.K, tuple(mc.D_NONZERO))


@functools.lru_cache(maxsize=None)
def _single_frame_results():
    d = _new_det()
    try:
        d.set_map(_lying_map())
        out = []
        for img in _batch_frames():
            corners, ids = d.detect_markers(img)
            pose, rob = d.map_pose_robust(camera=CAM_D, corners=corners, ids=ids, inlier_px=PX, min_markers=2)
            out.append((corners, ids, pose.copy(), rob.copy()))
        return out
    finally:
        d.close()


def test_four_outcomes_in_one_batch(det):
    want = _single_frame_results()
    assert [int(w[3]["status"]) for w in want] == [_lib.MAP_ROBUST_OK, _lib.MAP_ROBUST_OK, _lib.MAP_ROBUST_NO_CONSENSUS, _lib.MAP_ROBUST_NO_MARKERS]
    assert [int(w[3]["n_outliers"]) for w in want] == [0, 1, 4, 0] and [int(w[3]["n_used"]) for w in want] == [5, 6, 4, 0]
    assert map_robust_outlier_ids(want[1][3], want[1][1], _lying_map()["id"]).tolist() == [25]
    assert _zero_pose(want[2][2]) and _zero_pose(want[3][2]) and want[3][3]["hypothesis"] == -1
    det.set_map(_lying_map())
    for round_ in range(2):  # the second round: camera and options are known, the detect call runs the kernel in its own stream
        res = det.detect_markers_batch(_batch_frames())
        poses, robs = det.map_pose_robust_last(camera=CAM_D, inlier_px=PX, min_markers=2)
        assert len(poses) == len(robs) == 4
        for f in range(4):
            assert np.array_equal(res[f][0], want[f][0]) and np.array_equal(res[f][1], want[f][1])
            assert poses[f].tobytes() == want[f][2].tobytes() and robs[f].tobytes() == want[f][3].tobytes(), (round_, f)
    # other options: not a copy of what the detect call ran
    poses1, robs1 = det.map_pose_robust_last(camera=CAM_D, inlier_px=PX, min_markers=7)
    for f in range(4):
        pose, rob = det.map_pose_robust(camera=CAM_D, corners=want[f][0], ids=want[f][1], inlier_px=PX, min_markers=7)
        assert poses1[f].tobytes() == pose.tobytes() and robs1[f].tobytes() == rob.tobytes(), f
    assert robs1["status"].tolist() == [_lib.MAP_ROBUST_NO_CONSENSUS] * 3 + [_lib.MAP_ROBUST_NO_MARKERS]  # (no frame has seven markers)
    det.set_map(None)


def test_pose_ahead_equals_no_pose_ahead(monkeypatch):
    want = _single_frame_results()
    monkeypatch.setenv("FID_NO_POSE_AHEAD", "1")
    d = _new_det()
    try:
        d.set_map(_lying_map())
        for _ in range(2):
            d.detect_markers_batch(_batch_frames())
            poses, robs = d.map_pose_robust_last(camera=CAM_D, inlier_px=PX, min_markers=2)
            for f in range(4):
                assert poses[f].tobytes() == want[f][2].tobytes() and robs[f].tobytes() == want[f][3].tobytes(), f
    finally:
        d.close()


def test_the_submit_collect_ring_on_two_contexts():
    want = _single_frame_results()
    frames = np.ascontiguousarray(_batch_frames())
    dets = [_new_det() for _ in range(2)]
    try:
        for d in dets:
            d.set_map(_lying_map())
        dets[0].submit_batch(frames)
        for k in range(1, 5):
            dets[k % 2].submit_batch(frames, after=dets[(k - 1) % 2])
            d = dets[(k - 1) % 2]
            d.collect()
            with pytest.raises(FidError):
                dets[k % 2].map_pose_robust_last(camera=CAM_D, inlier_px=PX, min_markers=2)  # a batch is in flight there
            poses, robs = d.map_pose_robust_last(camera=CAM_D, inlier_px=PX, min_markers=2)
            for f in range(4):
                assert poses[f].tobytes() == want[f][2].tobytes() and robs[f].tobytes() == want[f][3].tobytes(), (k, f)
        dets[0].collect()
    finally:
        for d in dets:
            d.close()


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_with_two_map_entries_exchanged(det):
    """scene("3x2", 1) detected on the device; in the map the entries of ids 21 and 24 have exchanged places."""
    truthful = mc.scene_map("3x2")
    lying = truthful.copy()
    lying["R"][[1, 4]], lying["t"][[1, 4]] = truthful["R"][[4, 1]], truthful["t"][[4, 1]]
    fr = mc.scene("3x2", 1)
    cam = Camera(cm.PLUMB_BOB, mc.K, ())
    det.set_map(lying)
    corners, ids = det.detect_markers(fr.image)
    poses, robs = det.map_pose_robust_last(camera=cam, inlier_px=PX, min_markers=2)
    plain_lying = det.map_pose_last(camera=cam)[0].copy()
    assert sorted(map_robust_outlier_ids(robs[0], ids, lying["id"]).tolist()) == [21, 24]
    keep = [i for i, v in enumerate(ids.tolist()) if v not in (21, 24)]
    det.set_map(truthful)
    four = det.map_pose(camera=cam, corners=corners[keep], ids=ids[keep])
    assert poses[0].tobytes() == four.tobytes()
    R, t = mc.scene_pose("3x2", 1)

    def dist(p):
        return float(max(np.abs(p["R"] - R).max(), np.abs(p["tvec"] - t).max()))

    print("distance to scene_pose: robust", dist(poses[0]), "plain pose of the lying map", dist(plain_lying))
    assert dist(plain_lying) > dist(poses[0])
    det.set_map(None)


# ------------------------------------------------------------------------------------------------ refusals, and nothing else changes
def test_refusals(det):
    c = rc.cases()["floor8_3bad"]
    cam = _camera(c)
    det.set_map(None)
    with pytest.raises(FidError):  # no map
        det.map_pose_robust(camera=cam, corners=c.corners, ids=c.ids, inlier_px=PX)
    det.set_map(c.entries)
    for bad in (dict(inlier_px=0.0), dict(inlier_px=-1.0), dict(inlier_px=float("nan")), dict(inlier_px=float("inf")), dict(inlier_px=PX, min_markers=0)):
        with pytest.raises(FidError) as e:
            det.map_pose_robust(camera=cam, corners=c.corners, ids=c.ids, **bad)
        assert e.value.status == _lib.FID_E_INVALID_ARG
    with pytest.raises(ValueError):  # the ABI has no default
        det.map_pose_robust(camera=cam, corners=c.corners, ids=c.ids)
    pose, rob = det.map_pose_robust(camera=cam, corners=np.zeros((0, 4, 2), np.float32), ids=[], inlier_px=PX)
    assert rob["status"] == _lib.MAP_ROBUST_NO_MARKERS and _zero_pose(pose) and rob["n_used"] == 0
    # capacity: room for fewer frames than the last call had
    det.detect_markers_batch(_batch_frames())
    opts = _lib.FidMapRobustOpts(PX, 2, 0)
    import ctypes as C
    out, robs = np.zeros(4, MAP_POSE_DTYPE), np.zeros(4, MAP_ROBUST_DTYPE)
    assert det._L.fid_map_pose_robust_last_cam(det._ctx, C.byref(cam.c), C.byref(opts), out.ctypes.data, robs.ctypes.data, 3) == _lib.FID_E_CAPACITY
    det.set_map(None)


def test_a_robust_call_changes_nothing_else(det):
    """fid_detect, fid_pose_last_cam and fid_map_pose_last_cam return the bytes they returned before, with robust calls between."""
    frames = _batch_frames()
    det.set_map(_lying_map())

    def run(robust):
        blobs = []
        for _ in range(2):  # (the second round: whatever was asked for rides in the detect call)
            res = det.detect_markers_batch(frames)
            if robust:
                det.map_pose_robust_last(camera=CAM_D, inlier_px=PX, min_markers=2)
            mp = det.map_pose_last(camera=CAM_D)
            poses = det.pose_last(mc.SCENE_LEN, camera=CAM_D)
            if robust:
                det.map_pose_robust(camera=CAM_D, corners=res[1][0], ids=res[1][1], inlier_px=PX, min_markers=2)
                assert det.map_pose_last(camera=CAM_D).tobytes() == mp.tobytes()
            blobs.append(b"".join(r[0].tobytes() + r[1].tobytes() for r in res) + mp.tobytes() +
                         b"".join(p.rvecs.tobytes() + p.tvecs.tobytes() + p.image_error.tobytes() for p in poses))
        assert blobs[0] == blobs[1]
        return blobs[0]

    before = run(False)
    assert run(True) == before and run(False) == before
    det.set_map(None)
