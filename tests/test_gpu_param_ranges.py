"""The detector parameters aruco_detect's own surface accepts (cfg/DetectorParams.cfg, the pnh.param block of aruco_detect.cpp)
beyond the node defaults, up to the oracle's bounds: adaptive-threshold windows above 81 px (k_threshold_wide), cornerSubPix
windows 8..15 (k_subpix<15>), marker grids of up to 16 cells and unwarp patches of up to 256 px (k_identify).  Every stage
against the oracle under the same parameters, bit for bit; past the bounds the library keeps refusing.  Run on the MI355X: -m gpu."""
import numpy as np
import pytest

import oracle
from fiducials_amd import _lib
from fiducials_amd._lib import FidError
from fiducials_amd.detector import ArucoDetector, default_params
from fiducials_amd.dictionary import get_predefined_dictionary
from fiducials_amd.synth import make_frame
from helpers import n_scales
from test_gpu_parity import check_stages, params_pair

pytestmark = pytest.mark.gpu

# (min, max, step): every table has a window above 81 px
WIDE_TABLES = [(3, 101, 14), (83, 83, 1), (21, 255, 26), (5, 401, 44)]


def _dict(name):
    return get_predefined_dictionary(name, allow_fillers=True)  # (6x6 / 7x7: filler codewords, the same on both sides)


def _table(t):
    return dict(adaptiveThreshWinSizeMin=t[0], adaptiveThreshWinSizeMax=t[1], adaptiveThreshWinSizeStep=t[2])


def _same(a, b):
    assert a[1].tolist() == b[1].tolist()
    assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("dic", [7, 0])
@pytest.mark.parametrize("table", WIDE_TABLES)
def test_wide_threshold_windows_1080p(table, dic):
    """Threshold masks of every scale (check_stages: == oracle.adaptive_threshold) and every later stage, 1920 x 1080."""
    d = get_predefined_dictionary(dic)
    p, op = params_pair(**_table(table))
    assert max(p.adaptiveThreshWinSizeMin + s * p.adaptiveThreshWinSizeStep for s in range(n_scales(p))) > 81
    fr = make_frame(d, 4100 + table[1] + dic, n_markers=12, side_range=(150, 260))
    det = ArucoDetector(d, params=p, max_width=1920, max_height=1080)
    try:
        _, ids, _ = check_stages(det, fr.image, d, op)
        assert len(ids) >= 6
    finally:
        det.close()


def test_window_wider_and_taller_than_the_frame():
    """One 301-px window on a 96 x 64 frame: the replicated border is most of every box."""
    d = get_predefined_dictionary(0)
    fr = make_frame(d, 4200, width=96, height=64, n_markers=1, side_range=(26, 29), max_tilt_deg=10)
    p, op = params_pair(**_table((301, 301, 1)))
    det = ArucoDetector(d, params=p, max_width=96, max_height=64)
    try:
        check_stages(det, fr.image, d, op)
        masks = det.tap_masks(1, 1, 64, 96)[0]
        assert 0 < (masks[0] > 0).sum() < 96 * 64  # (not a trivial mask)
    finally:
        det.close()


def test_wide_windows_batch_forms():
    """detect_markers_batch and submit_batch + collect over 8 frames: frame f == a single-frame call on frame f == the oracle."""
    d = get_predefined_dictionary(6)
    p, op = params_pair(**_table((21, 255, 26)))
    frames = np.stack([make_frame(d, 4300 + i, width=1280, height=720, n_markers=8, side_range=(120, 200)).image for i in range(8)])
    det = ArucoDetector(d, params=p, max_width=1280, max_height=720, max_batch=8)
    try:
        batch = det.detect_markers_batch(frames)
        det.submit_batch(frames)
        sub = det.collect()
        found = 0
        for f in range(8):
            single = det.detect_markers(frames[f])
            oids, ocorners = oracle.detect(frames[f], d, params=op)
            _same(batch[f], single)
            _same(sub[f], single)
            _same(single, (ocorners, oids))
            found += len(oids)
        assert found >= 40
    finally:
        det.close()


@pytest.mark.parametrize("iters", [30, 100])
@pytest.mark.parametrize("win", [8, 11, 15])
def test_subpix_windows_up_to_15(win, iters):
    """cornerRefinementWinSize 8..15 (k_subpix<15>): pre-subpix and final corners == the oracle's."""
    d = get_predefined_dictionary(6)
    p, op = params_pair(cornerRefinementWinSize=win, cornerRefinementMaxIterations=iters)
    fr = make_frame(d, 4400 + win, width=1280, height=720, n_markers=10, side_range=(110, 200))
    det = ArucoDetector(d, params=p, max_width=1280, max_height=720)
    try:
        _, ids, ocorners = check_stages(det, fr.image, d, op)
        assert len(ids) >= 6
        assert not np.array_equal(det.tap_presubpix()[0][:len(ids)]["corners"].reshape(-1, 4, 2), ocorners)  # (corners moved)
    finally:
        det.close()


# (dictionary, markerBorderBits, perspectiveRemovePixelPerCell): grids of 10 to 16 cells, patches of 161 and 252 px
WIDE_GRIDS = [("DICT_6X6_250", 2, 8), ("DICT_6X6_250", 5, 8), ("DICT_7X7_1000", 2, 8), ("DICT_7X7_1000", 4, 8), ("DICT_4X4_50", 6, 8),
              ("DICT_5X5_1000", 1, 23), ("DICT_5X5_1000", 1, 36)]


def _grid_params(bb, cell):
    # (borders of 2 cells and more: the outline of the synthetic frames' one-cell white quiet zone lies within 5 % of the marker's perimeter,
    #  and _filterTooCloseCandidates would keep that outline instead of the marker; 2 % keeps both)
    kw = dict(markerBorderBits=bb, perspectiveRemovePixelPerCell=cell)
    if bb >= 2:
        kw["minMarkerDistanceRate"] = 0.02
    return kw


@pytest.mark.parametrize("case", WIDE_GRIDS, ids=[f"{n}-b{b}-c{c}" for n, b, c in WIDE_GRIDS])
def test_wide_grids_and_large_patches(case):
    """Grids up to 16 cells a side and unwarp patches up to 256 px: bits, ident, ids and corners == the oracle's, 1080p."""
    name, bb, cell = case
    d = _dict(name)
    p, op = params_pair(**_grid_params(bb, cell))
    msb = d.marker_size + 2 * bb
    assert msb > 9 or msb * cell > 160  # (both refused before: 9 cells, 160 px)
    fr = make_frame(d, 505, n_markers=20, side_range=(120, 180), border_bits=bb, max_tilt_deg=20)
    det = ArucoDetector(d, params=p, max_width=1920, max_height=1080)
    try:
        _, ids, _ = check_stages(det, fr.image, d, op)
        assert det.tap_bits().shape[-2:] == (msb, msb)
        assert len(set(ids.tolist()) & set(fr.ids.tolist())) >= 15  # the oracle (== the library) finds most of the 20
    finally:
        det.close()


def test_reconfigure_to_widened_ranges_and_back():
    """dynamic_reconfigure on a live context: defaults -> each widened setting -> defaults.  After every step the results equal a
    fresh context's and the oracle's; what lies past the bounds is refused and the context keeps its parameters."""
    steps = [
        ("DICT_6X6_250", 1, dict(**_table((5, 401, 44)))),
        ("DICT_6X6_250", 1, dict(cornerRefinementWinSize=15, cornerRefinementMaxIterations=100)),
        ("DICT_6X6_250", 5, _grid_params(5, 8)),
        ("DICT_7X7_1000", 4, _grid_params(4, 8)),
        ("DICT_5X5_1000", 1, _grid_params(1, 36)),
    ]
    refused = {
        "DICT_6X6_250": [(dict(cornerRefinementWinSize=16), _lib.FID_E_INVALID_ARG)],
        "DICT_7X7_1000": [(dict(markerBorderBits=5), _lib.FID_E_UNSUPPORTED)],  # 17 cells
        "DICT_5X5_1000": [(dict(perspectiveRemovePixelPerCell=37), _lib.FID_E_UNSUPPORTED)],  # 259-px patch
    }
    dets = {}
    try:
        for name, bb, kw in steps:
            d = _dict(name)
            if name not in dets:
                dets[name] = ArucoDetector(d, max_width=1920, max_height=1080)
            det = dets[name]
            fr = make_frame(d, 505 if bb >= 2 else 4600 + bb, n_markers=20, side_range=(120, 180), border_bits=bb, max_tilt_deg=20)
            p, op = params_pair(**kw)
            det.set_params(p)
            got = check_stages(det, fr.image, d, op)
            fresh = ArucoDetector(d, params=p, max_width=1920, max_height=1080)
            try:
                _same(got[:2], fresh.detect_markers(fr.image))
            finally:
                fresh.close()
            assert len(got[1]) >= 10
            for bad, status in refused.get(name, []):
                q, _ = params_pair(**{**kw, **bad})
                with pytest.raises(FidError) as e:
                    det.set_params(q)
                assert e.value.status == status
                assert "at most" in str(e.value)  # (fid_last_error names the bound)
                check_stages(det, fr.image, d, op)  # still the accepted parameters
            # ... and back to the defaults
            det.set_params(default_params())
            base = make_frame(d, 4700, n_markers=20)
            check_stages(det, base.image, d)
    finally:
        for det in dets.values():
            det.close()


def test_creation_past_the_bounds_is_refused():
    """fid_create refuses what lies past the widened ranges (never an unchecked result)."""
    for name, kw, status in [("DICT_6X6_250", dict(cornerRefinementWinSize=16), _lib.FID_E_INVALID_ARG),
                             ("DICT_7X7_1000", dict(markerBorderBits=5), _lib.FID_E_UNSUPPORTED),
                             ("DICT_5X5_1000", dict(perspectiveRemovePixelPerCell=37), _lib.FID_E_UNSUPPORTED),
                             ("DICT_4X4_50", _table((3, 16385, 16382)), _lib.FID_E_UNSUPPORTED)]:
        p, _ = params_pair(**kw)
        with pytest.raises(FidError) as e:
            ArucoDetector(_dict(name), params=p, max_width=640, max_height=480)
        assert e.value.status == status
