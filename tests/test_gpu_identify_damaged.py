"""k_identify where it has something to decide: damaged markers and sparse histograms (frames of tests/identify_cases.py).

Every other GPU test feeds the kernel clean codewords on dense histograms.  Here every frame goes through check_stages against
the oracle's trace under the same parameters -- threshold masks, candidates, FILTERED corners, the BITS tap, the IDENT tap (id and
rotation), pre-subpix and final ids and corners, all np.array_equal, overflow flags zero -- and then, independently of the oracle,
against the plain numpy rule of identify_cases.py marker by marker: the id the FIRST table entry within capacity gives, nothing
returned beyond the correction capacity or the border limit.  All comparisons are exact; there is no tolerance in this file.
tests/test_identify_cases.py (CPU) shows for every frame used here that each drawn marker reaches identification.

  family 1  11 frames x 12 markers, Hamming distance 0 ... maxCorr + 1 in each: 2-, 4- (uint4 path), 5- and 7-byte codewords
  family 2  4 frames x 8 markers: first entry within capacity across lanes, 64-marker rounds and the second 256-marker fetch
  family 3  12 frames x 8 markers: border errors 0, limit - 1, limit, limit + 1 under markerBorderBits = 2
  family 4  32 flat scenes x 6 markers, minOtsuStdDev 0 and 5: two or three occupied histogram bins on the 64-bin word edges
  batches   2 x 3 frames through one detect_markers_batch call on a max_batch = 4 context, and through single calls"""
import numpy as np
import pytest

import identify_cases as ic
from fiducials_amd.detector import ArucoDetector
from helpers import n_scales
from test_gpu_parity import check_stages, params_pair
from test_gpu_seedless_probe import FrameOfBatch

pytestmark = pytest.mark.gpu


def run_case(det, case, op):
    corners, ids, _ = check_stages(det, case.image, case.d, op)
    ic.check_against_rule(case, ids, corners)
    return corners, ids


def run_alone(case):
    p, op = params_pair(**case.params)
    w, h = case.size
    det = ArucoDetector(case.d, params=p, max_width=w, max_height=h)
    try:
        return run_case(det, case, op)
    finally:
        det.close()


@pytest.mark.parametrize("k", range(len(ic.FAMILY1)), ids=[f"{n}-{r}" for n, r in ic.FAMILY1])
def test_data_bit_errors_at_the_capacity_edge(k):
    case = ic.family1_case(k)
    corners, ids = run_alone(case)
    assert len(ids) == case.counts()[1] and case.counts()[2] >= 1


@pytest.mark.parametrize("k", range(len(ic.FAMILY2)), ids=[f"{n}x{n}-{'with70' if w else 'no70'}" for n, w in ic.FAMILY2])
def test_first_entry_within_capacity_across_rounds_and_lanes(k):
    case = ic.family2_case(k)
    corners, ids = run_alone(case)
    assert sorted(ids.tolist()) == sorted(case.wanted)


@pytest.mark.parametrize("k", range(len(ic.FAMILY3)), ids=[f"{n}-{r}" for n, r in ic.FAMILY3])
def test_border_errors_at_the_limit(k):
    case = ic.family3_case(k)
    corners, ids = run_alone(case)
    assert len(ids) == case.counts()[1] and case.counts()[2] >= 2


@pytest.mark.parametrize("levels", ic.F4_LEVELS + ic.F4_LEVELS3, ids=lambda lv: "-".join(map(str, lv)))
def test_sparse_histograms(levels):
    """One level triple: flat and rotated scene, minOtsuStdDev 0 and the default 5, on one context."""
    cases = [ic.family4_case(k) for k, (lv, rot, sd) in enumerate(ic.FAMILY4) if lv == levels]
    assert len(cases) == 4
    w, h = cases[0].size
    det = ArucoDetector(cases[0].d, max_width=w, max_height=h)
    try:
        for case in cases:
            p, op = params_pair(**case.params)
            det.set_params(p)
            corners, ids = run_case(det, case, op)
            if case.must_read:
                assert sorted(ids.tolist()) == sorted(ic.F4_IDS)
            if case.uniform:
                assert len(ids) == 0
    finally:
        det.close()


@pytest.mark.parametrize("group", ic.BATCH_GROUPS)
def test_the_same_frames_through_the_batch_path(group):
    """k_identify's worklist carries (frame, candidate) pairs of three frames; every frame as in its single call."""
    d, params, cases = ic.batch_group(group)
    p, op = params_pair(**params)
    w, h = cases[0].size
    frames = np.stack([c.image for c in cases])
    det = ArucoDetector(d, params=p, max_width=w, max_height=h, max_batch=4)
    try:
        results = det.detect_markers_batch(frames)
        masks = det.tap_masks(len(cases), n_scales(op), h, w)
        for f, case in enumerate(cases):
            check_stages(FrameOfBatch(det, f, results, masks), frames[f], d, op)
            ic.check_against_rule(case, results[f][1], results[f][0])
        for f, case in enumerate(cases):
            corners, ids = run_case(det, case, op)
            assert ids.tolist() == results[f][1].tolist() and np.array_equal(corners, results[f][0])
    finally:
        det.close()
