"""k_threshold_stream's mask parking and the walkers' register allocation (round 9).

The consumer waves of k_threshold_stream park the mask word pairs of their rows in lanes of registers and store them in groups of
rows, a row per lane; the shapes here are chosen for such groups and lanes, at 64 rows a group as at 16: heights at and around the
detector's floor of 8 rows and around multiples of 16 (17, 33, 47, 64, 79), widths of one strip (64), up to a strip's edge (191),
one column past it (193) and with a last wave partly outside the image (450), batches of 1 and 3, and row segments (FID_THR_ROWS) of
20 and 36 rows -- multiples of 4 but not of 16, so that a segment starts in the middle of a group of rows -- and the five-wave
strips (FID_THR_NW=5) once.  Frames are random gray with a few dark rectangles, so that every scale sets and clears bits.  All 13
masks `==` the oracle's.

One more case runs tests/test_gpu_chain_codes.py's frame as a 16-frame call through the default path: the walkers, whose register
allocation this round changed (fid_kernels.hip, WALKER_WG_ATTR), still produce `==` candidates.  Run on the MI355X: -m gpu."""
import numpy as np
import pytest

import oracle
from fiducials_amd.detector import ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary
from helpers import n_scales
from test_gpu_chain_codes import check_candidates, shapes_frame

pytestmark = pytest.mark.gpu

D4 = get_predefined_dictionary("DICT_4X4_50")
HEIGHTS = [8, 9, 15, 16, 17, 33, 47, 64, 79]
WIDTHS = [64, 191, 193, 450]
NFRAMES = 3
ENVS = [{}, {"FID_THR_ROWS": "20"}, {"FID_THR_ROWS": "36"}, {"FID_THR_NW": "5"}]

_cache = {}


def _frames(w, h):
    rng = np.random.default_rng(1000 * w + h)
    fr = rng.integers(0, 256, (NFRAMES, h, w), dtype=np.uint8)
    for f in range(NFRAMES):
        for _ in range(4):  # dark rectangles of every size up to the frame's: the wide windows see them too
            x0, y0 = int(rng.integers(0, w - 2)), int(rng.integers(0, h - 2))
            x1, y1 = int(rng.integers(x0 + 2, w + 1)), int(rng.integers(y0 + 2, h + 1))
            fr[f, y0:y1, x0:x1] = rng.integers(0, 40, (y1 - y0, x1 - x0), dtype=np.uint8)
    return fr


def _case(w, h):
    """Frames of one shape and the oracle's masks of every frame and scale: computed once, shared by every variant, never written."""
    if (w, h) not in _cache:
        p = oracle.default_params()
        fr = _frames(w, h)
        wins = [p.adaptiveThreshWinSizeMin + s * p.adaptiveThreshWinSizeStep for s in range(n_scales(p))]
        assert len(wins) == 13
        want = np.stack([np.stack([oracle.adaptive_threshold(fr[f], win, p.adaptiveThreshConstant) > 0 for win in wins])
                         for f in range(NFRAMES)])
        assert all(0 < want[:, s].mean() < 1 for s in range(13)), (w, h)  # (every scale sets bits, and not all of them)
        fr.setflags(write=False)
        want.setflags(write=False)
        _cache[(w, h)] = (fr, want)
    return _cache[(w, h)]


@pytest.mark.parametrize("env", ENVS, ids=[",".join(f"{k}={v}" for k, v in e.items()) or "default" for e in ENVS])
def test_masks_equal_the_oracle(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    det = ArucoDetector(D4, max_width=max(WIDTHS), max_height=max(HEIGHTS), max_batch=NFRAMES)
    try:
        assert n_scales(det.params) == 13  # (the node's table: k_threshold_stream)
        for w in WIDTHS:
            for h in HEIGHTS:
                fr, want = _case(w, h)
                for n in (1, NFRAMES):
                    det.detect_markers_batch(fr[:n])
                    got = det.tap_masks(n, 13, h, w) > 0
                    assert got.shape == want[:n].shape
                    if not np.array_equal(got, want[:n]):
                        bad = np.argwhere(got != want[:n])
                        raise AssertionError(f"{w}x{h} batch {n} {env}: {len(bad)} px differ, first (frame, scale, y, x) = {bad[0].tolist()}")
    finally:
        det.close()


def test_walkers_candidates_16_frame_call():
    img = shapes_frame(5)
    _, _, tr = oracle.detect(img, get_predefined_dictionary(6), trace=True)
    assert len(tr["initial"]["scale"]) >= 20
    det = ArucoDetector(6, max_width=img.shape[1], max_height=img.shape[0], max_batch=16)
    try:
        det.detect_markers_batch(np.stack([img] * 16))
        for f in (0, 5, 15):
            cnt = det.tap_counts()[f]
            check_candidates(det.tap_candidates(False)[f][:cnt[2]], cnt, tr)
    finally:
        det.close()
