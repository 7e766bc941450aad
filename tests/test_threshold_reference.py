"""The adaptive-threshold reference (helpers.adaptive_threshold_ref, int64 numpy) against brute force, and the oracle against it at
every window the library accepts, up to FID_MAX_THR_WIN = 2 * 8191 + 1.  No GPU."""
import numpy as np
import pytest

import oracle
from helpers import adaptive_threshold_ref

# the oracle's int32 path ends at 2049 (2 * sum + area <= 511 * win^2 < 2^31); 2897 is the first window whose area passes 2^23
WINDOWS = [3, 7, 51, 81, 83, 401, 2049, 2051, 2053, 2897, 2899, 4097, 16383]
SIZES = [(8, 8), (96, 64), (1000, 37), (37, 1000)]  # (width, height)


def _clamped_counts(n, r):
    """WY[y, i]: how often row i falls in the clamped window y - r .. y + r."""
    wy = np.zeros((n, n), np.int64)
    for y in range(n):
        np.add.at(wy[y], np.clip(np.arange(y - r, y + r + 1), 0, n - 1), 1)
    return wy


def _frames(w, h, seed):
    """All 255 with a darker square, noise, a horizontal and a vertical ramp, half-bright noise: the largest box sums and the
    closest calls."""
    rng = np.random.default_rng(seed)
    sq = np.full((h, w), 255, np.uint8)
    sq[h // 4:h // 4 + max(h // 2, 1), w // 4:w // 4 + max(w // 2, 1)] = 200
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    hramp = np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8), (h, w)).copy()
    vramp = np.broadcast_to((np.arange(h) * 255 // max(h - 1, 1)).astype(np.uint8)[:, None], (h, w)).copy()
    half = noise.copy()
    if w >= h:
        half[:, w // 2:] = 250
    else:
        half[h // 2:] = 250
    return {"square": sq, "noise": noise, "hramp": hramp, "vramp": vramp, "half": half}


@pytest.mark.parametrize("win", [3, 51, 83, 301, 2049, 2051, 4097, 16383])
@pytest.mark.parametrize("shape", [(8, 8), (13, 29), (40, 50)])  # (height, width)
def test_reference_equals_bruteforce(shape, win):
    """S = WY @ G @ WX^T in exact int64; mean = round(S / area); foreground iff src - mean <= -floor(C)."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    frames = [rng.integers(0, 256, shape, dtype=np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)]
    sq = np.full(shape, 255, np.uint8)
    sq[h // 4:3 * h // 4, w // 4:3 * w // 4] = 200
    frames.append(sq)
    r, area = win // 2, win * win
    wy, wx = _clamped_counts(h, r), _clamped_counts(w, r)
    for g in frames:
        s = wy @ g.astype(np.int64) @ wx.T
        assert s.max() <= 255 * area
        for c in (7.0, 7.5, -0.5, 0.0):
            mean = (2 * s + area) // (2 * area)
            want = np.where(g.astype(np.int64) - mean <= -int(np.floor(c)), 255, 0)
            assert np.array_equal(adaptive_threshold_ref(g, win, c), want), (win, c)
    # an even window is win + 1
    assert np.array_equal(adaptive_threshold_ref(frames[0], win - 1, 7.0), adaptive_threshold_ref(frames[0], win, 7.0))


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("win", WINDOWS)
def test_oracle_equals_reference(win, size):
    """oracle.adaptive_threshold (ora_adaptive_threshold) == the int64 reference at every accepted window, including those
    where 2 * sum + area passes 2^31 on a bright frame (win >= 2051)."""
    w, h = size
    for name, g in _frames(w, h, win + w).items():
        for c in (7.0, 7.5, -0.5):
            ref = adaptive_threshold_ref(g, win, c)
            got = oracle.adaptive_threshold(g, win, c)
            assert np.array_equal(got > 0, ref > 0), f"{name} C={c}: {(got > 0) != (ref > 0)} px differ"


def test_a_bright_frame_with_a_square_at_the_widest_windows():
    """The first case the int32 oracle got wrong: 255 with a 20 x 20 square of 200 is 400 foreground pixels at any window."""
    g = np.full((40, 50), 255, np.uint8)
    g[10:30, 15:35] = 200
    for win in (2049, 2051, 2053, 16383):
        ref = adaptive_threshold_ref(g, win, 7.0)
        assert (ref > 0).sum() == 400
        assert np.array_equal(oracle.adaptive_threshold(g, win, 7.0), ref)


def test_double_scale_rounding_equals_exact_above_2_23():
    """boxFilter's ColumnSum<int, uchar> sums in CV_64F once win^2 > 2^23 and rounds s * (1 / area) with cvRound.  For every odd
    window from 2897 (the first above 2^23) to 16383, sums on either side of every half-step, floor((k + 1/2) area) + {-1, 0, 1}
    for k = 0 .. 254, round exactly: the oracle's integer round(sum / area) restates that path too."""
    wins = np.arange(2897, 16384, 2, dtype=np.int64)
    areas = wins * wins
    assert areas[0] > 1 << 23 and (2895 * 2895) <= 1 << 23
    k = np.arange(255, dtype=np.int64)
    for a in np.array_split(areas, 16):
        half = (2 * k[None, :] + 1) * a[:, None] // 2  # floor((k + 1/2) area)
        s = (half[:, :, None] + np.array([-1, 0, 1])).reshape(len(a), -1)
        exact = (2 * s + a[:, None]) // (2 * a[:, None])
        dbl = np.rint(s.astype(np.float64) * (1.0 / a.astype(np.float64))[:, None]).astype(np.int64)
        assert np.array_equal(exact, dbl)
