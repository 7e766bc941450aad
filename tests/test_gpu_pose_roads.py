"""The roads by which a pose question is answered (fid_api.hip: PoseRequest): computed behind the detect call, computed ahead in the
next detect call's stream, or copied from what is at hand -- and every way in which what is at hand stops being the answer: a new
frame, another camera, another fiducial_len / sigma_px / inlier_px / min_markers, another map, a batch in flight.

Five requests: the marker pose, the marker pose with its covariance, the map pose, the map pose with its covariance, the map pose by
consensus.  Every comparison is tobytes() equality against a fresh context that detects once and is asked once (no tolerance), and the
sequences run with looking ahead switched on and off (FID_NO_POSE_AHEAD).  Frames: the 4- and 3-marker synthetic frames of
test_gpu_pose_cov.py and the rendered "2x2" scene with its map; contexts of max_batch 2, max_markers 16."""
import ctypes as C
import functools

import numpy as np
import pytest

import aruco_map_cases as mc
import camera_model_cases as cm
import pose_cases as pc
from fiducials_amd import _lib
from fiducials_amd.camera import Camera
from fiducials_amd.detector import MAP_POSE_COV_DTYPE, MAP_POSE_DTYPE, MAP_ROBUST_DTYPE, POSE_COV_DTYPE, ArucoDetector, FidError, _MARKER_DT, _POSE_DT
from test_gpu_pose_cov import _frames as _pose_cov_frames

pytestmark = pytest.mark.gpu

MM = 16
LEN, LEN2 = 0.14, 0.2
PX = _lib.MAP_ROBUST_INLIER_PX
CAM1 = Camera(cm.PLUMB_BOB, mc.K, pc.dist_coeffs("mild"))
K2 = np.array([[481.3, 0.0, 324.5], [0.0, 478.9, 236.0], [0.0, 0.0, 1.0]])
CAM2 = Camera(cm.RATIONAL, K2, cm.SETS["prism12"][1])  # (another model and another K)
IN_FLIGHT = "a submitted batch is in flight: fid_collect first"
_frames = functools.lru_cache(maxsize=None)(_pose_cov_frames)  # (the 4-, 3- and 1-marker frames, rendered once)


def _pose_records(d):
    mm = d.max_markers
    return np.concatenate([d._poses_np[f * mm:f * mm + max(int(d._n[f]), 0)] for f in range(d._last_frames)])


def _ask_pose(d, cam, length=LEN):
    d.pose_last(length, camera=cam, unpack=False)
    return (_pose_records(d),)


def _ask_pose_cov(d, cam, sigma=1.0):
    _, covs = d.pose_cov_last(LEN, camera=cam, sigma_px=sigma)
    return _pose_records(d), np.concatenate(covs)


def _ask_map(d, cam):
    return (d.map_pose_last(camera=cam),)


def _ask_map_cov(d, cam, sigma=1.0):
    return d.map_pose_cov_last(camera=cam, sigma_px=sigma)


def _ask_robust(d, cam, opts=(PX, 2)):
    return d.map_pose_robust_last(camera=cam, inlier_px=opts[0], min_markers=opts[1])


class Request:
    """One kind of question: how it is asked, the other values of its second key, the plain question beside a covariance one, and
    which frames it is asked about ("markers": the synthetic frames, "scene": the 2x2 scene under two camera poses)."""

    def __init__(self, name, ask, keys2, frames, plain=None):
        self.name, self.ask, self.keys2, self.frames, self.plain = name, ask, keys2, frames, plain

    def __repr__(self):
        return self.name


POSE = Request("pose", _ask_pose, (LEN2,), "markers")
POSE_COV = Request("pose_cov", _ask_pose_cov, (2.0,), "markers", plain=POSE)
MAP = Request("map_pose", _ask_map, (), "scene")
MAP_COV = Request("map_pose_cov", _ask_map_cov, (2.0,), "scene", plain=MAP)
# (another inlier_px alone: so narrow that the corners of a rendered frame do not all agree; another min_markers alone: more than the scene has)
ROBUST = Request("map_pose_robust", _ask_robust, ((0.02, 2), (PX, 5)), "scene")
REQUESTS = [POSE, POSE_COV, MAP, MAP_COV, ROBUST]
MAP_REQUESTS = [MAP, MAP_COV, ROBUST]


def _image(name):
    if name in ("A_markers", "B_markers"):
        return _frames()[0 if name[0] == "A" else 1].image
    if name in ("A_scene", "B_scene"):
        return mc.scene("2x2", 1 if name[0] == "A" else 2).image
    assert name == "batch"  # (the scene's 4 markers and the 3-marker frame)
    return np.ascontiguousarray(np.stack([mc.scene("2x2", 1).image, _frames()[1].image]))


def _moved_map():
    e = mc.scene_map("2x2").copy()
    e["t"][1][0] += 0.005  # (one entry moved by 5 mm)
    return e


MAPS = {"2x2": lambda: mc.scene_map("2x2"), "moved": _moved_map}


def _new_det(emap="2x2"):
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=2, max_markers=MM)
    if emap:
        d.set_map(MAPS[emap]())
    return d


def _detect(d, name):
    return d.detect_markers_batch(_image(name)) if name == "batch" else d.detect_markers(_image(name))


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


_FRESH = {}


def fresh(req, frame, cam, key=None, emap="2x2"):
    """What a context made for the question answers: one detect call, asked once.  Computed once per question, never changed."""
    k = (req.name, frame, id(cam), key, emap)
    if k not in _FRESH:
        d = _new_det(emap)
        try:
            _detect(d, frame)
            _FRESH[k] = tuple(np.array(x) for x in (req.ask(d, cam) if key is None else req.ask(d, cam, key)))
            for x in _FRESH[k]:
                x.setflags(write=False)
        finally:
            d.close()
    return _FRESH[k]


@pytest.fixture(params=[True, False], ids=["ahead", "no_ahead"])
def ahead(request, monkeypatch):
    if not request.param:
        monkeypatch.setenv("FID_NO_POSE_AHEAD", "1")
    return request.param


@pytest.mark.parametrize("req", REQUESTS, ids=repr)
def test_the_sequence_of_questions(req, ahead):
    """Computed now, then looked ahead on the same frame; a new frame; another camera and back; another second key."""
    A, B = "A_" + req.frames, "B_" + req.frames
    d = _new_det()
    try:
        _detect(d, A)
        first = req.ask(d, CAM1)  # computed behind the detect call
        assert _same(first, fresh(req, A, CAM1))
        _detect(d, A)
        assert _same(req.ask(d, CAM1), first)  # looked ahead (or computed again): the same bytes
        _detect(d, B)
        assert _same(req.ask(d, CAM1), fresh(req, B, CAM1)) and not _same(fresh(req, B, CAM1), first)  # a new frame: its answer
        # another camera: that camera's answer, the same after another detect call, and the first camera's answer again
        assert _same(req.ask(d, CAM2), fresh(req, B, CAM2)) and not _same(fresh(req, B, CAM2), fresh(req, B, CAM1))
        _detect(d, B)
        assert _same(req.ask(d, CAM2), fresh(req, B, CAM2))
        assert _same(req.ask(d, CAM1), fresh(req, B, CAM1))
        for key2 in req.keys2:
            # another second key, asked where the first one's answer is at hand; then looked ahead; then the first key again
            _detect(d, B)
            other = req.ask(d, CAM1, key2)
            assert _same(other, fresh(req, B, CAM1, key2)) and not _same(other, fresh(req, B, CAM1)), key2
            _detect(d, B)
            assert _same(req.ask(d, CAM1, key2), other), key2
            assert _same(req.ask(d, CAM1), fresh(req, B, CAM1)), key2
        if req.plain is not None:
            # sigma_px 1 -> 2: the same poses, every covariance entry four times as large, exactly
            one = fresh(req, B, CAM1)
            assert other[0].tobytes() == one[0].tobytes()
            cov1, cov2 = (one[1], other[1]) if req is POSE_COV else (one[1]["pose"], other[1]["pose"])
            assert len(cov1) > 0 and (cov1["status"] == 0).all()
            for field in ("cov_rt", "cov_pose", "sigma2"):
                assert np.array_equal(cov2[field], 4.0 * cov1[field]), field
            if req is MAP_COV:
                assert np.array_equal(other[1]["cov_cam_pose"], 4.0 * one[1]["cov_cam_pose"])
    finally:
        d.close()


def test_the_look_ahead_shows_in_the_pose_stage_time(monkeypatch):
    """The one place the look-ahead is observable from the API: under FID_PROFILE the detect call that computes the remembered pose
    reports a pose stage time; a context that never asked reports zero."""
    monkeypatch.setenv("FID_PROFILE", "1")
    asked, never = _new_det(None), _new_det(None)
    try:
        for d in (asked, never):
            _detect(d, "A_markers")
        _ask_pose(asked, CAM1)
        for d in (asked, never):
            _detect(d, "A_markers")
        assert asked.stage_ms()["pose"] > 0.0 and never.stage_ms()["pose"] == 0.0
        assert _same(_ask_pose(asked, CAM1), fresh(POSE, "A_markers", CAM1))
    finally:
        asked.close()
        never.close()


@pytest.mark.parametrize("req", [POSE_COV, MAP_COV], ids=repr)
def test_plain_after_covariance(req, ahead):
    """The plain question where the covariance one is remembered: the usual bytes; the covariance asked again after the next detect
    call has its earlier bytes."""
    A = "A_" + req.frames
    d = _new_det()
    try:
        _detect(d, A)
        with_cov = req.ask(d, CAM1)
        _detect(d, A)
        assert _same(req.plain.ask(d, CAM1), fresh(req.plain, A, CAM1))
        assert with_cov[0].tobytes() == fresh(req.plain, A, CAM1)[0].tobytes()
        _detect(d, A)
        assert _same(req.ask(d, CAM1), with_cov) and _same(with_cov, fresh(req, A, CAM1))
    finally:
        d.close()


@pytest.mark.parametrize("req", MAP_REQUESTS, ids=repr)
def test_another_map_between_detect_and_question(req, ahead):
    """fid_set_map with one entry moved, between a detect call that computed the remembered request and the question: the new map's
    answer.  An empty map: refused with its message."""
    d = _new_det()
    try:
        _detect(d, "A_scene")
        assert _same(req.ask(d, CAM1), fresh(req, "A_scene", CAM1))
        _detect(d, "A_scene")
        d.set_map(_moved_map())
        moved = req.ask(d, CAM1)
        assert _same(moved, fresh(req, "A_scene", CAM1, emap="moved")) and not _same(moved, fresh(req, "A_scene", CAM1))
        _detect(d, "A_scene")
        assert _same(req.ask(d, CAM1), moved)
        d.set_map(None)
        with pytest.raises(FidError) as e:
            req.ask(d, CAM1)
        assert e.value.status == _lib.FID_E_INVALID_ARG and "no map: fid_set_map first" in str(e.value)
    finally:
        d.close()


def _raw_calls(d, cam, markers):
    """Every _last and every _cam entry point by its C signature, writing into arrays the caller hands in: name -> (sizes in bytes of
    the output arrays, call).  cap: frames (the map requests) or markers per frame (the pose requests) the arrays have room for."""
    L, ctx, c, n = d._L, d._ctx, C.byref(cam.c), len(markers)
    opts = C.byref(_lib.FidMapRobustOpts(PX, 2, 0))
    P, PC, M, MC, R = _POSE_DT.itemsize, POSE_COV_DTYPE.itemsize, MAP_POSE_DTYPE.itemsize, MAP_POSE_COV_DTYPE.itemsize, MAP_ROBUST_DTYPE.itemsize
    pose = lambda a: C.cast(C.c_void_p(a), C.POINTER(_lib.FidPoseOut))  # noqa: E731
    mk = C.cast(C.c_void_p(markers.ctypes.data), C.POINTER(_lib.FidMarker))
    return {
        "fid_pose_last_cam": ((2 * MM * P,), lambda o, cap=MM: L.fid_pose_last_cam(ctx, c, LEN, pose(o[0]), cap)),
        "fid_pose_last_cov_cam": ((2 * MM * P, 2 * MM * PC), lambda o, cap=MM: L.fid_pose_last_cov_cam(ctx, c, LEN, pose(o[0]), cap, 1.0, o[1])),
        "fid_map_pose_last_cam": ((2 * M,), lambda o, cap=2: L.fid_map_pose_last_cam(ctx, c, o[0], cap)),
        "fid_map_pose_last_cov_cam": ((2 * M, 2 * MC), lambda o, cap=2: L.fid_map_pose_last_cov_cam(ctx, c, o[0], cap, 1.0, o[1])),
        "fid_map_pose_robust_last_cam": ((2 * M, 2 * R), lambda o, cap=2: L.fid_map_pose_robust_last_cam(ctx, c, opts, o[0], o[1], cap)),
        "fid_pose_cam": ((n * P,), lambda o: L.fid_pose_cam(ctx, c, mk, None, n, LEN, pose(o[0]))),
        "fid_pose_cov_cam": ((n * P, n * PC), lambda o: L.fid_pose_cov_cam(ctx, c, mk, None, n, LEN, pose(o[0]), 1.0, o[1])),
        "fid_map_pose_cam": ((M,), lambda o: L.fid_map_pose_cam(ctx, c, markers.ctypes.data, n, o[0])),
        "fid_map_pose_cov_cam": ((M, MC), lambda o: L.fid_map_pose_cov_cam(ctx, c, markers.ctypes.data, n, o[0], 1.0, o[1])),
        "fid_map_pose_robust_cam": ((M, R), lambda o: L.fid_map_pose_robust_cam(ctx, c, markers.ctypes.data, n, opts, o[0], o[1])),
    }


def _marker_list(corners, ids):
    mk = np.zeros(len(ids), _MARKER_DT)
    mk["id"], mk["corners"] = ids, np.asarray(corners, np.float32).reshape(len(ids), 8)
    return mk


def _last_error(d):
    return (d._L.fid_last_error(d._ctx) or b"").decode()


def test_every_entry_point_is_refused_in_flight(ahead):
    """While a batch is submitted every _last and every _cam entry point returns FID_E_INVALID_ARG and leaves the caller's arrays as
    they were; after fid_collect the five questions have the answers of a context that was asked about the batch once."""
    d = _new_det()
    try:
        corners, ids = _detect(d, "A_scene")
        markers = _marker_list(corners, ids)
        for req in REQUESTS:
            req.ask(d, CAM1)  # (all five remembered: the batch computes them in its stream)
        batch = _image("batch")
        d.submit_batch(batch)
        for name, (sizes, call) in _raw_calls(d, CAM1, markers).items():
            outs = [np.full(s, 7, np.uint8) for s in sizes]
            assert call([o.ctypes.data for o in outs]) == _lib.FID_E_INVALID_ARG, name
            assert all((o == 7).all() for o in outs), name
            if name not in ("fid_pose_cam", "fid_pose_cov_cam"):  # (those two: test_pose_cam_refused_in_flight_says_why)
                assert _last_error(d) == IN_FLIGHT, name
        found = d.collect()
        assert [len(i) for _, i in found] == [4, 3]
        for req in REQUESTS:
            assert _same(req.ask(d, CAM1), fresh(req, "batch", CAM1)), req
    finally:
        d.close()


def test_pose_cam_refused_in_flight_says_why():
    """fid_pose_cam and fid_pose_cov_cam refused in flight set the message every other entry point sets.  (Before the entry points
    shared their guards these two returned FID_E_INVALID_ARG without a message: this is the one test of this file that the code
    before that change does not pass.)"""
    for name in ("fid_pose_cam", "fid_pose_cov_cam"):
        d = _new_det()
        try:
            corners, ids = _detect(d, "A_scene")
            markers = _marker_list(corners, ids)
            d.submit_batch(_image("batch"))
            sizes, call = _raw_calls(d, CAM1, markers)[name]
            outs = [np.full(s, 7, np.uint8) for s in sizes]
            assert call([o.ctypes.data for o in outs]) == _lib.FID_E_INVALID_ARG and _last_error(d) == IN_FLIGHT, name
            d.collect()
        finally:
            d.close()


def test_capacity(ahead):
    """Room for fewer frames than the batch had: FID_E_CAPACITY with its message, for the three map requests.  Room for fewer markers
    per frame than a frame has: FID_E_CAPACITY and the truncated copy, for the two pose requests."""
    d = _new_det()
    try:
        assert [len(i) for _, i in _detect(d, "batch")] == [4, 3]
        calls = _raw_calls(d, CAM1, np.zeros(0, _MARKER_DT))
        for turn in range(2):  # (computed behind the detect call, then -- remembered by the full-size questions below -- looked ahead)
            for name in ("fid_map_pose_last_cam", "fid_map_pose_last_cov_cam", "fid_map_pose_robust_last_cam"):
                sizes, call = calls[name]
                outs = [np.full(s, 7, np.uint8) for s in sizes]
                assert call([o.ctypes.data for o in outs], 1) == _lib.FID_E_CAPACITY, name
                assert _last_error(d) == "caller room for 1 frames, the last call had 2", name
                assert all((o == 7).all() for o in outs), name
            cap = 3
            want = fresh(POSE_COV, "batch", CAM1)
            for name in ("fid_pose_last_cam", "fid_pose_last_cov_cam"):
                sizes, call = calls[name]
                outs = [np.full(s, 7, np.uint8) for s in sizes]
                assert call([o.ctypes.data for o in outs], cap) == _lib.FID_E_CAPACITY, name
                poses = outs[0].view(_POSE_DT)
                assert poses[:3].tobytes() == want[0][:3].tobytes() and poses[cap:cap + 3].tobytes() == want[0][4:7].tobytes(), name
                assert (outs[0][2 * cap * _POSE_DT.itemsize:] == 7).all(), name
                if len(outs) > 1:
                    cov = outs[1].view(POSE_COV_DTYPE)
                    assert cov[:3].tobytes() == want[1][:3].tobytes() and cov[cap:cap + 3].tobytes() == want[1][4:7].tobytes(), name
            for req in REQUESTS:
                assert _same(req.ask(d, CAM1), fresh(req, "batch", CAM1)), req
            _detect(d, "batch")
    finally:
        d.close()


HOST_LISTS = {
    "map_pose": lambda d, mk: (d.map_pose(corners=mk["corners"], ids=mk["id"], camera=CAM1),),
    "map_pose_cov": lambda d, mk: d.map_pose_cov(corners=mk["corners"], ids=mk["id"], camera=CAM1, sigma_px=1.0),
    "map_pose_robust": lambda d, mk: d.map_pose_robust(corners=mk["corners"], ids=mk["id"], camera=CAM1, inlier_px=PX, min_markers=2),
}


@pytest.mark.parametrize("req", MAP_REQUESTS, ids=repr)
def test_host_lists_between_the_batch_records(req):
    """A _cam call on a list from the host between a detect call and its _last question leaves that answer as it was (the list's
    result has a slot of its own behind the batch's).  Lists of 3, 300 and 3 markers -- the staging buffer grows past its 256-marker
    step and is then reused -- each have the answer of a context made for that list."""
    call = HOST_LISTS[req.name]
    d = _new_det()
    try:
        corners, ids = _detect(d, "A_scene")
        four = _marker_list(corners, ids)
        lists = [four[:3], np.tile(four, 75), four[1:]]
        want = []
        for mk in lists:
            f = _new_det()
            try:
                want.append(tuple(np.array(x) for x in call(f, mk)))
            finally:
                f.close()
        assert not _same(want[0], want[2])
        answer = req.ask(d, CAM1)
        assert _same(answer, fresh(req, "A_scene", CAM1))
        _detect(d, "A_scene")
        for mk, w in zip(lists, want):
            assert _same(tuple(np.array(x) for x in call(d, mk)), w), len(mk)
            assert _same(req.ask(d, CAM1), answer), len(mk)
    finally:
        d.close()
