"""ChArUco diamonds on the device (include/fid_abi.h: "ChArUco diamonds"; fid_diamond.hip) against the NumPy restatement, stage by stage:
the diamonds, their members and their order, the positions to 2 float ulps, the windows recomputed from the device's own positions, the
refined corners bit for bit against oracle.corner_subpix started where the device started; the calls on the last detect call against
the call that brings its input from the host, byte for byte; the pose against fid_pose_cam on the equivalent markers.

corners0 against the restatement (exact homographies, where the device uses the closed form), measured on the MI355X: 0.0 ulps on
every case (2 allowed, the board tests' allowance)."""
import ctypes as C
import functools

import numpy as np
import pytest

import charuco_restatement as cr
import diamond_cases as dc
import diamond_restatement as dr
from fiducials_amd import _lib
from fiducials_amd.detector import ArucoDetector, FidError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(dc.DICT, max_width=dc.W, max_height=dc.H, max_batch=4, max_markers=64)
    yield d
    d.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_records(got, want, ids, corners, image, rate, refine=True):
    """DIAMOND_DTYPE records held to the restatement's; returns the worst ulps of corners0"""
    assert [g["index"].tolist() for g in got] == [w["index"].tolist() for w in want]
    assert [g["ids"].tolist() for g in got] == [w["ids"].tolist() for w in want]
    L = dr.layout(rate)
    worst = 0.0
    for g, w in zip(got, want):
        worst = max(worst, dc.ulps(g["corners0"], w["corners0"]).max())
        wins = [dr.device_window(L, corners, g["index"].tolist(), i, g["corners0"][r]) for r, i in enumerate(dr.RECORD_CORNERS)]
        assert g["win"].tolist() == wins
        if refine:
            ref = cr.refine(image, g["corners0"], g["win"])
            assert np.array_equal(_bits(ref), _bits(g["corners"]))
        else:
            assert np.array_equal(_bits(g["corners"]), _bits(g["corners0"]))
    assert worst <= 2.0, worst
    return worst


def _check_case(det, c):
    img = c.image
    got = det.diamonds_detect(c.corners, c.ids, img, c.rate, c.max_rep_rate)
    worst = _check_records(got, c.want, c.ids, c.corners, img, c.rate)
    raw = det.diamonds_detect(c.corners, c.ids, img, c.rate, c.max_rep_rate, refine=False)
    _check_records(raw, c.want, c.ids, c.corners, img, c.rate, refine=False)
    assert raw["corners0"].tobytes() == got["corners0"].tobytes() and raw["win"].tobytes() == got["win"].tobytes()
    if c.truth is not None and len(got):
        moved = np.abs(got["corners"] - got["corners0"]).max()
        err = max(np.abs(g["corners"] - t).max() for g, t in zip(got, c.truth))
        print(c.name, "refinement moved the corners by up to %.3f px; refined corners within %.3f px of the truth" % (moved, err))
        assert err < 0.5  # (the picture is the hand-made list's own)
    print(c.name, "markers", len(c.ids), "diamonds", len(got), "corners0: worst %.3g ulps" % worst)
    return got, worst


# ------------------------------------------------------------------------------------------------ the kernels on hand-made markers
@pytest.mark.parametrize("roll", dc.ROLLS)
def test_one_diamond_tilted_and_rolled(det, roll):
    got, _ = _check_case(det, dc.case_one(roll))
    assert len(got) == 1 and got[0]["ids"].tolist() == list(dc.ONE_IDS) and got[0]["win"].tolist() == [10] * 4


def test_two_diamonds_and_loose_markers_shuffled(det):
    """Every anchor comes after its partners in the list: a partner tried as an anchor founds nothing and assigns nothing."""
    c = dc.case_two()
    got, _ = _check_case(det, c)
    assert [g["ids"].tolist() for g in got] == [[3, 3, 9, 3], [10, 11, 12, 13]] and [int(g["index"][0]) for g in got] == [9, 11]
    # the list in another order: the same diamonds, each with the same members
    o = np.random.default_rng(5).permutation(len(c.ids))
    again = det.diamonds_detect(c.corners[o], c.ids[o], c.image, c.rate)
    assert sorted(sorted(o[g["index"]].tolist()) for g in again) == sorted(sorted(g["index"].tolist()) for g in got)


def test_three_of_four_markers_are_no_diamond(det):
    got, _ = _check_case(det, dc.case_three_of_four())
    assert len(got) == 0


def test_four_equal_ids(det):
    got, _ = _check_case(det, dc.case_equal_ids())
    assert len(got) == 1 and got[0]["ids"].tolist() == [77] * 4 and got[0]["index"].tolist() == [0, 1, 2, 3]


def test_a_corner_inside_the_margin_drops_the_diamond_and_keeps_its_markers(det):
    c = dc.case_margin()
    got, _ = _check_case(det, c)
    assert len(got) == 0
    # without the first anchor its copy founds the diamond, whose corners are all selected
    alone = det.diamonds_detect(c.corners[1:], c.ids[1:], c.image, c.rate)
    assert len(alone) == 1 and alone[0]["index"].tolist() == [3, 0, 1, 2] and alone[0]["corners0"][:, 0].min() > 2.05
    # ... and the first anchor alone with the partners: found, one corner at x = 1.8, not reported
    assert len(det.diamonds_detect(c.corners[:4], c.ids[:4], c.image, c.rate)) == 0


def test_more_markers_than_lanes(det):
    """68 noise-free markers, 17 diamonds: more than one pass of 64 markers and of 16 diamonds"""
    c = dc.case_17()
    got, _ = _check_case(det, c)
    assert len(got) == 17 and sorted(got["index"].reshape(-1).tolist()) == list(range(68))


def test_both_limits_and_the_callers_room(det):
    """256 noise-free markers, 64 diamonds: FID_DIAMOND_MAX_MARKERS and FID_DIAMOND_MAX_PER_FRAME; then room for fewer than found"""
    c = dc.case_64()
    got, _ = _check_case(det, c)
    assert len(got) == 64 and sorted(got["index"].reshape(-1).tolist()) == list(range(256))
    with pytest.raises(FidError) as e:
        det.diamonds_detect(c.corners, c.ids, c.image, c.rate, cap=10)
    assert e.value.status == _lib.FID_E_CAPACITY and det.last_diamond_counts.value == 64
    c17 = dc.case_17()
    with pytest.raises(FidError) as e:
        det.diamonds_detect(c17.corners, c17.ids, c17.image, c17.rate, cap=16)
    assert e.value.status == _lib.FID_E_CAPACITY and det.last_diamond_counts.value == 17
    with pytest.raises(FidError) as e:  # one marker more than the kernels stage
        det.diamonds_detect(np.concatenate([c.corners, c.corners[:1] + 300]), np.concatenate([c.ids, [999]]), c.image, c.rate)
    assert e.value.status == _lib.FID_E_UNSUPPORTED and "FID_DIAMOND_MAX_MARKERS" in str(e.value)


def test_the_tolerance_is_the_options(det):
    """one partner 0.9 and 1.1 tolerances away (the hand-enumerated diamond of the CPU tests), and a larger max_rep_rate that takes it"""
    m, s, x0, y0 = 40.0, 80.0, 100.0, 60.0

    def sq(sx, sy):
        x, y = x0 + sx * s + (s - m) / 2, y0 + (2 - sy) * s + (s - m) / 2
        return [[x, y], [x + m, y], [x + m, y + m], [x, y + m]]

    corners = np.array([sq(1, 0), sq(0, 1), sq(2, 1), sq(1, 2)], np.float32)
    ids = np.array([10, 11, 12, 13], np.int32)
    img = dc.frontal_frame().image
    for dx, rep, n in ((36.0, 1.0, 1), (44.0, 1.0, 0), (44.0, 1.2, 1), (0.0, 0.01, 1)):
        moved = corners.copy()
        moved[1] += np.float32([dx, 0.0])
        want, mg = dr.detect(2.0, rep, ids, moved, dc.W, dc.H)
        assert mg.worst() >= dc.MIN_MARGIN and len(want) == n
        got = det.diamonds_detect(moved, ids, img, 2.0, rep)
        _check_records(got, want, ids, moved, img, 2.0)
    got = det.diamonds_detect(corners, ids, img, 2.0, refine=False)
    assert np.abs(got[0]["corners0"] - [[180, 140], [260, 140], [260, 220], [180, 220]]).max() < 1e-3


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _batch_frames():
    frames = np.stack([dc.two_frame().image, dc.one_frame(37.0).image, dc.frontal_frame().image, dc.one_frame(90.0).image])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _single_frame_results():
    """per frame: (corners, ids, diamonds_last, diamonds_last without refinement), each from a single-frame call"""
    d = ArucoDetector(dc.DICT, max_width=dc.W, max_height=dc.H, max_batch=4, max_markers=64)
    try:
        out = []
        for img in _batch_frames():
            corners, ids = d.detect_markers(img)
            out.append((corners, ids, d.diamonds_last(dc.RATE)[0], d.diamonds_last(dc.RATE, refine=False)[0]))
        return out
    finally:
        d.close()


def test_a_rendered_frame_end_to_end(det):
    """detect_markers -> diamonds_last == diamonds_detect on the returned markers, byte for byte; the diamonds are the picture's"""
    want = _single_frame_results()
    frames = (dc.two_frame(), dc.one_frame(37.0), dc.frontal_frame(), dc.one_frame(90.0))
    for img, fr, (corners, ids, last, raw) in zip(_batch_frames(), frames, want):
        assert det.diamonds_detect(corners, ids, img, dc.RATE).tobytes() == last.tobytes()
        assert det.diamonds_detect(corners, ids, img, dc.RATE, refine=False).tobytes() == raw.tobytes()
        rest, mg = dr.detect(dc.RATE, 1.0, ids, corners, dc.W, dc.H)
        assert mg.worst() >= dc.MIN_MARGIN
        _check_records(last, rest, ids, corners, img, dc.RATE)
        assert sorted(g["ids"].tolist() for g in last) == sorted(b.ids.tolist() for b, _, _ in fr.diamonds)
        for g in last:
            k = [b.ids.tolist() for b, _, _ in fr.diamonds].index(g["ids"].tolist())
            truth = fr.corners_image[k]
            side = np.linalg.norm(truth - np.roll(truth, 1, axis=0), axis=1).min()
            assert np.linalg.norm(g["corners"] - truth, axis=1).max() < side / 4
    assert [len(w[2]) for w in want] == [2, 1, 1, 1]


def test_a_batch_equals_the_single_frame_calls(det):
    want = _single_frame_results()
    frames = np.ascontiguousarray(_batch_frames())
    for how in ("batch", "submit"):
        if how == "batch":
            res = det.detect_markers_batch(frames)
        else:
            det.submit_batch(frames)
            with pytest.raises(FidError) as e:
                det.diamonds_last(dc.RATE)  # a batch is in flight
            assert e.value.status == _lib.FID_E_INVALID_ARG and "in flight" in str(e.value)
            res = det.collect()
        last, raw = det.diamonds_last(dc.RATE), det.diamonds_last(dc.RATE, refine=False)
        assert len(last) == len(raw) == 4
        for f in range(4):
            assert np.array_equal(res[f][0], want[f][0]) and np.array_equal(res[f][1], want[f][1])
            assert last[f].tobytes() == want[f][2].tobytes() and raw[f].tobytes() == want[f][3].tobytes(), (how, f)
    with pytest.raises(FidError) as e:
        det.diamonds_last(dc.RATE, cap=1)
    assert e.value.status == _lib.FID_E_CAPACITY and det.last_diamond_counts.tolist() == [2, 1, 1, 1]


# ------------------------------------------------------------------------------------------------ the pose
def test_the_pose_is_fid_pose_cam_on_the_equivalent_markers(det):
    want = _single_frame_results()
    Z5 = np.zeros(5)
    for fr, (_, _, last, _) in zip((dc.two_frame(), dc.one_frame(37.0)), want):
        got = det.diamond_pose(last, dc.SQUARE, dc.K, Z5)
        same = det.estimate_pose_single_markers(last["corners"], last["ids"][:, 0], dc.SQUARE, camera=_camera(Z5))
        for name in ("rvecs", "tvecs", "image_error", "object_error", "fiducial_area"):
            assert np.asarray(getattr(got, name)).tobytes() == np.asarray(getattr(same, name)).tobytes(), name
        for i, g in enumerate(last):
            k = [b.ids.tolist() for b, _, _ in fr.diamonds].index(g["ids"].tolist())
            b, R, t = fr.diamonds[k]
            err = np.abs(got.tvecs[i] - (R @ b.centre + t)).max()
            print("diamond", g["ids"].tolist(), "tvec within %.4f m of the truth" % err)
            assert err < 0.02  # (the board tests' tolerance against the picture's pose)
    assert len(det.diamond_pose(np.zeros(0, _lib.DIAMOND_DTYPE), dc.SQUARE, dc.K, Z5).tvecs) == 0
    with pytest.raises(FidError):
        det.diamond_pose(want[0][2], 0.0, dc.K, Z5)


def _camera(D):
    from fiducials_amd.camera import Camera
    return Camera(_lib.CAM_PLUMB_BOB, dc.K, D)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(det):
    L, ctx = det._L, det._ctx
    c = dc.case_one(0.0)
    fresh = ArucoDetector(dc.DICT, max_width=dc.W, max_height=dc.H, max_batch=1, max_markers=64)
    try:
        with pytest.raises(FidError) as e:
            fresh.diamonds_last(dc.RATE)
        assert e.value.status == _lib.FID_E_INVALID_ARG and "no last call" in str(e.value)
    finally:
        fresh.close()
    det.detect_markers(dc.frontal_frame().image)
    for rate, word in ((1.0, "square_marker_rate"), (0.5, "square_marker_rate"), (np.inf, "square_marker_rate"), (np.nan, "square_marker_rate")):
        with pytest.raises(FidError) as e:
            det.diamonds_detect(c.corners, c.ids, c.image, rate)
        assert e.value.status == _lib.FID_E_INVALID_ARG and word in str(e.value) and "above 1" in str(e.value)
        with pytest.raises(FidError) as e:
            det.diamonds_last(rate)
        assert e.value.status == _lib.FID_E_INVALID_ARG and word in str(e.value)
    for rep in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(FidError) as e:
            det.diamonds_detect(c.corners, c.ids, c.image, dc.RATE, rep)
        assert e.value.status == _lib.FID_E_INVALID_ARG and "max_rep_rate" in str(e.value) and "above 0" in str(e.value)
        with pytest.raises(FidError) as e:
            det.diamonds_last(dc.RATE, rep)
        assert e.value.status == _lib.FID_E_INVALID_ARG and "max_rep_rate" in str(e.value)
    o = _lib.FidDiamondOpts()
    L.fid_default_diamond_opts(C.byref(o))
    assert (o.square_marker_rate, o.max_rep_rate, o.refine) == (0.04 / 0.024, 1.0, 1)
    n = np.zeros(4, np.int32)
    out = np.zeros(4, _lib.DIAMOND_DTYPE)
    assert L.fid_diamonds_last(ctx, C.byref(o), None, 4, n.ctypes.data) == _lib.FID_E_INVALID_ARG  # a NULL output
    assert L.fid_diamonds_last(ctx, C.byref(o), out.ctypes.data, 4, None) == _lib.FID_E_INVALID_ARG
    assert L.fid_diamonds_last(ctx, None, out.ctypes.data, 4, n.ctypes.data) == _lib.FID_E_INVALID_ARG
    assert b"NULL" in L.fid_last_error(ctx)
    assert L.fid_diamonds_last(ctx, C.byref(o), out.ctypes.data, 4, n.ctypes.data) == _lib.FID_OK and n[0] == 1
    img = np.ascontiguousarray(c.image)
    mk = np.zeros(4, [("id", "<i4"), ("corners", "<f4", (8,))])
    mk["id"], mk["corners"] = c.ids, c.corners.reshape(4, 8)
    nn = C.c_int32(0)
    args = (mk.ctypes.data, 4, img.ctypes.data, dc.W, dc.H, dc.W)
    assert L.fid_diamonds_detect(ctx, C.byref(o), *args, None, 4, C.byref(nn)) == _lib.FID_E_INVALID_ARG
    assert L.fid_diamonds_detect(ctx, C.byref(o), *args, out.ctypes.data, 4, None) == _lib.FID_E_INVALID_ARG
    assert L.fid_diamonds_detect(ctx, C.byref(o), mk.ctypes.data, 4, img.ctypes.data, dc.W + 8, dc.H, dc.W + 8, out.ctypes.data, 4, C.byref(nn)) == _lib.FID_E_INVALID_ARG
    assert b"frame limits" in L.fid_last_error(ctx)
    assert L.fid_diamonds_detect(ctx, C.byref(o), *args, out.ctypes.data, 4, C.byref(nn)) == _lib.FID_OK and nn.value == 1
    # the call from the host leaves the last call's results as they are
    assert L.fid_diamonds_last(ctx, C.byref(o), out.ctypes.data, 4, n.ctypes.data) == _lib.FID_OK and n[0] == 1
    assert out[0]["ids"].tolist() == list(dc.ONE_IDS)
    wide = ArucoDetector(dc.DICT, max_width=dc.W, max_height=dc.H, max_batch=1, max_markers=512)
    try:
        wide.detect_markers(dc.frontal_frame().image)
        with pytest.raises(FidError) as e:
            wide.diamonds_last(dc.RATE)
        assert e.value.status == _lib.FID_E_UNSUPPORTED and "max_markers_per_frame" in str(e.value)
    finally:
        wide.close()


def test_a_detector_that_never_asks_is_as_before(det):
    """Markers and fid_last_launches the same on a detector that never asked for diamonds, and on one before and after it asked."""
    frames = np.ascontiguousarray(_batch_frames())

    def run(d):
        res = d.detect_markers_batch(frames)
        return b"".join(r[0].tobytes() + r[1].tobytes() for r in res), d.last_launches()

    never = ArucoDetector(dc.DICT, max_width=dc.W, max_height=dc.H, max_batch=4, max_markers=64)
    try:
        plain = run(never)
    finally:
        never.close()
    before = run(det)
    assert len(det.diamonds_last(dc.RATE)) == 4
    assert det.last_launches() == before[1]
    after = run(det)
    assert plain == before == after
