"""Device buffers that grow and are then reused (fid_devmem.h behind the feature entry points): ONE context answers a small, a larger
and again the small request of a feature, and each answer equals -- byte for byte -- that of a context made fresh for that request.
The pattern of test_host_lists_between_the_batch_records (tests/test_gpu_pose_roads.py), which covers the growth of the map calls'
marker list; here the calibration blocks (sized by views) and their input arrays, the map builder's one block with its robust part
behind the plain one, the ChArUco and diamond staging (image and marker list), and the cell-bits array that fid_set_params grows.
The requests and the call helpers are those of the features' own test files; what an answer must BE is checked there."""
import functools

import numpy as np
import pytest

import calib_cases as cc
import charuco_calib_cases as ccc
import charuco_cases as chc
import diamond_cases as dc
import map_build_cases as mc
import map_build_robust_cases as mrc
import oracle
import test_gpu_calibrate as tcal
import test_gpu_charuco_calibrate as tchcal
import test_gpu_map_build as tb
import test_gpu_map_build_robust as tbr
from fiducials_amd import _lib
from fiducials_amd.detector import ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary
from fiducials_amd.synth import make_frame
from test_gpu_parity import params_pair


def _bytes(x):
    """An answer (nested tuples of arrays, records, cameras and numbers) as bytes."""
    if isinstance(x, (tuple, list)):
        return b"|".join(_bytes(v) for v in x)
    if hasattr(x, "c") and hasattr(x.c, "K"):  # a camera.Camera
        return tcal.k16_of_cam(x).tobytes()
    return np.ascontiguousarray(x).tobytes()


def _hold(make, run, requests):
    """requests: [(name, request)].  One context made by make() answers them in order; each answer is that of a fresh context."""
    want = {}
    for name, r in requests:
        if name not in want:
            f = make()
            try:
                want[name] = _bytes(run(f, r))
            finally:
                f.close()
    assert len(set(want.values())) == len(want), "the requests must have different answers"
    d = make()
    try:
        for k, (name, r) in enumerate(requests):
            assert _bytes(run(d, r)) == want[name], (k, name)
    finally:
        d.close()


@pytest.mark.gpu
def test_calibrate_map_views_shrink_grow_shrink():
    """3 views of 6 markers, 17 views of 1, 3 of 6: the view block grows with the second call while its marker array does not (18, 17,
    18 records), and the third call runs in the block the second left."""
    def run(det, shape):
        c = cc.case("plumb_bob", shape)
        det.set_map(c["entries"])
        res = tcal.calibrate(det, c["views"], c["image_size"], tcal.cam_of(c["model"], cc.zero_start(c), c["n_dist"]), c["free"])
        assert res[0] == _lib.FID_OK, det._L.fid_last_error(det._ctx)
        return res

    _hold(lambda: ArucoDetector(dictionary=6, max_width=640, max_height=480, max_batch=8, max_markers=64), run,
          [(s, s) for s in ("3x6", "17x1", "3x6")])


@pytest.mark.gpu
def test_calibrate_charuco_smallest_largest_smallest():
    """3 views of the 5 x 4 board's 12 corners, 5 views of the 22 x 23 board's 462, 3 of 12: views and records per view both grow."""
    def run(det, shape):
        c = ccc.case("plumb_bob", shape)
        det.set_charuco_board(ccc.device_board(c["board"]))
        res = tchcal.calibrate(det, c["views"], c["image_size"], tchcal.cam_of(c["model"], cc.zero_start(c), c["n_dist"]), c["free"])
        assert res[0] == _lib.FID_OK, det._L.fid_last_error(det._ctx)
        return res

    _hold(lambda: ArucoDetector(dictionary=ccc.DICT, max_width=640, max_height=480, max_batch=8, max_markers=64), run,
          [(s, s) for s in ("3x12", "5x462_exact", "3x12")])


@pytest.mark.gpu
def test_build_map_plain_larger_robust_plain():
    """chain3_min1, size22, the trimmed build of `swap` (its part of the block lies behind the plain part), chain3_min1 again."""
    def run(det, req):
        kind, name = req
        if kind == "robust":
            res = tbr.build_robust(det, mrc.case(name))
        else:
            res = tb.build(det, mc.case(name))
        assert res[0] == _lib.FID_OK, det._L.fid_last_error(det._ctx)
        return res

    _hold(lambda: ArucoDetector(dictionary=6, max_width=640, max_height=480, max_batch=12, max_markers=64), run,
          [("chain3_min1", ("plain", "chain3_min1")), ("size22", ("plain", "size22")), ("swap", ("robust", "swap")),
           ("chain3_min1", ("plain", "chain3_min1"))])


def _cropped(img):
    return np.ascontiguousarray(img[:img.shape[0] - 16, :img.shape[1] - 32])


@pytest.mark.gpu
def test_charuco_interpolate_image_and_list_grow():
    """A 608 x 464 image with 3 of the board's markers, the 640 x 480 image with the board's 10 and 290 markers of other ids (the list
    grows past its 256-marker step), then the first request again; with and without a camera."""
    fr = chc.view("tilted")
    R, t = chc.board_pose("5x4", *chc.VIEWS["tilted"])
    ids, corners = chc.hand_markers("5x4", R, t, seed=41)
    rng = np.random.default_rng(42)
    other_ids = (500 + np.arange(290)).astype(np.int32)
    other = (rng.uniform(40, 400, (290, 1, 2)) + np.array([[0, 0], [20, 0], [20, 20], [0, 20]])).astype(np.float32)
    small = (ids[:3], corners[:3], _cropped(fr.image))
    large = (np.concatenate([other_ids[:150], ids, other_ids[150:]]), np.concatenate([other[:150], corners, other[150:]]), fr.image)

    def run(det, req):
        i, c, img = req
        det.set_charuco_board(chc.board("5x4"))
        hom = det.charuco_interpolate(c, i, img, min_markers=1)
        cam = det.charuco_interpolate(c, i, img, min_markers=1, K=chc.K, D=np.zeros(5))
        assert len(hom) > 0 and len(cam) > 0
        return hom, cam

    _hold(lambda: ArucoDetector(chc.DICT, max_width=chc.W, max_height=chc.H, max_batch=4, max_markers=64), run,
          [("small", small), ("large", large), ("small", small)])


@pytest.mark.gpu
def test_diamonds_detect_image_grows():
    """one diamond on a 608 x 464 image, 64 diamonds (256 markers: all the staging holds) on the 640 x 480 one, the first again."""
    one, many = dc.case_one(0.0), dc.case_64()

    def run(det, req):
        c, img = req
        got = det.diamonds_detect(c.corners, c.ids, img, c.rate, c.max_rep_rate)
        assert len(got) == len(c.want)
        return got, det.diamonds_detect(c.corners, c.ids, img, c.rate, c.max_rep_rate, refine=False)

    _hold(lambda: ArucoDetector(dc.DICT, max_width=dc.W, max_height=dc.H, max_batch=4, max_markers=64), run,
          [("one", (one, _cropped(one.image))), ("64", (many, many.image)), ("one", (one, _cropped(one.image)))])


# ---- fid_set_params: the cell-bits array has room for grids of up to 9 cells; a 5 x 5 dictionary with a border of 3 has 11
BITS_SIZE = (384, 272)
BITS_TABLES = ((), (("markerBorderBits", 3),), ())


@functools.lru_cache(maxsize=None)
def _bits_frame(border_bits):
    fr = make_frame(get_predefined_dictionary(6), 700 + border_bits, width=BITS_SIZE[0], height=BITS_SIZE[1], n_markers=2, side_range=(70.0, 100.0),
                    max_tilt_deg=20.0, border_bits=border_bits)
    fr.image.setflags(write=False)
    return fr.image


@functools.lru_cache(maxsize=None)
def _bits_want(border_bits, table):
    _, op = params_pair(**dict(table))
    ids, corners = oracle.detect(_bits_frame(border_bits), get_predefined_dictionary(6), op)
    return ids, corners


def test_the_oracle_finds_the_wide_border_markers():
    """(no GPU) each frame has markers under its own parameters: the detect calls below have something to identify"""
    assert len(_bits_want(1, ())[0]) >= 1 and len(_bits_want(3, BITS_TABLES[1])[0]) >= 1


@pytest.mark.gpu
def test_detect_after_set_params_grows_the_cell_bits():
    """markerBorderBits 1 -> 3 -> 1 on one context (7, 11 and 7 cells a side): under every setting both frames -- the one drawn with
    that border and the other -- give the oracle's markers, ids and corners to the last bit."""
    d = ArucoDetector(6, params=params_pair()[0], max_width=BITS_SIZE[0], max_height=BITS_SIZE[1], max_batch=2, max_markers=32)
    try:
        for k, table in enumerate(BITS_TABLES):
            if k:
                d.set_params(params_pair(**dict(table))[0])
            for border in (1, 3):
                corners, ids = d.detect_markers(_bits_frame(border))
                oids, ocorners = _bits_want(border, table)
                assert ids.tolist() == oids.tolist(), (k, border)
                assert corners.dtype == ocorners.dtype and np.array_equal(corners, ocorners), (k, border)
    finally:
        d.close()
