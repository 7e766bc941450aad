import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def gold_json():
    return json.load(open(os.path.join(GOLD, "golden.json")))


def load_gray(key):
    return np.load(os.path.join(GOLD, key + ".npz"))["gray"]


def n_scales(p):
    return (p.adaptiveThreshWinSizeMax - p.adaptiveThreshWinSizeMin) // p.adaptiveThreshWinSizeStep + 1


def nested_same_id_frame(d, marker_id=3, width=1280, height=720, big_cell=84, small_cell=6, seed=9):
    """A frame on which `_filterDetectedMarkers` (aruco.cpp; called inside aruco::detectMarkers, aruco_detect.cpp:350) has
    something to remove: a large rendering of marker `marker_id` with small renderings of the SAME id pasted into the middle of
    white cells, so the same id is identified several times with one quad inside another."""
    from fiducials_amd.dictionary import draw_marker

    rng = np.random.default_rng(seed)
    n = d.marker_size + 2
    img = np.full((height, width), 190, np.uint8)
    side = big_cell * n
    big = draw_marker(d, marker_id, side)
    x0, y0 = (width - side) // 2, (height - side) // 2
    q = big_cell  # white quiet zone
    img[y0 - q:y0 + side + q, x0 - q:x0 + side + q] = 255
    img[y0:y0 + side, x0:x0 + side] = big
    bits = d.bits(marker_id)
    ss = small_cell * n
    small = draw_marker(d, marker_id, ss)
    placed = 0
    for r in range(d.marker_size):
        for c in range(d.marker_size):
            if bits[r, c] and placed < 2:
                cx = x0 + (c + 1) * big_cell + (big_cell - ss) // 2
                cy = y0 + (r + 1) * big_cell + (big_cell - ss) // 2
                img[cy:cy + ss, cx:cx + ss] = small
                placed += 1
    assert placed >= 1
    img = np.clip(img.astype(np.int32) + rng.integers(-2, 3, img.shape), 0, 255).astype(np.uint8)
    return img


def _box_sums_1d(a, r):
    """Sums along axis 0 of a over the clamped window y - r .. y + r (BORDER_REPLICATE), exact in int64.  The rows that fall off
    the frame are counted in closed form, so the memory is O(a.size) whatever r is."""
    n = a.shape[0]
    pre = np.zeros((n + 1,) + a.shape[1:], np.int64)
    np.cumsum(a, axis=0, out=pre[1:])
    y = np.arange(n)
    lo, hi = np.maximum(y - r, 0), np.minimum(y + r, n - 1)
    above = np.maximum(r - y, 0).reshape((n,) + (1,) * (a.ndim - 1))
    below = np.maximum(y + r - (n - 1), 0).reshape((n,) + (1,) * (a.ndim - 1))
    return pre[hi + 1] - pre[lo] + above * a[0] + below * a[n - 1]


def adaptive_threshold_ref(gray, win, C):
    """adaptiveThreshold(gray, 255, ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY_INV, win, C) as aruco calls it, in int64 numpy: the
    box sum S of a win x win BORDER_REPLICATE window, mean = round(S / win^2) (exact: never a tie for odd win), and foreground
    (255) iff src - mean <= -floor(C).  Even windows become win + 1 (aruco.cpp _threshold).  Independent of the oracle."""
    g = np.asarray(gray).astype(np.int64)
    if win % 2 == 0:
        win += 1
    r, area = win // 2, win * win
    s = _box_sums_1d(_box_sums_1d(g, r).T, r).T
    mean = (2 * s + area) // (2 * area)
    return np.where(g - mean <= -int(np.floor(C)), 255, 0).astype(np.uint8)
