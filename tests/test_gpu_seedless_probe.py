"""The seedless chain of a batch (a call of 16 frames or more) has two roads for its probes:
  FID_PROBE_PASSES=2   k_probe_lut<6, 0> + k_probe_refill<32, 1>   (starts -> surv1 -> surv)
  FID_PROBE_PASSES=1   k_probe_refill<32, 2>                        (starts -> surv in one pass; the default)
Both must give the oracle's stages on every frame of the call (test_gpu_parity.check_stages, frame by frame), and they must agree
with each other tap by tap.  The frames are drawn for what can go wrong between a probe of 6 steps, a probe of 32 steps and the
survivor walk behind them -- all shapes dark on light, no noise, so that every threshold mask's foreground is a subset of the
drawn pixels and a shape drawn clear of the 128-px grid lines has no seed state at any scale:
  * outer borders that close at 5, 6, 7 and at 31, 32, 33 points, hole borders at 6, 7 and 31, 32, 33 (a hole border of 5 points
    does not exist: a hole of one pixel has 4 border points, of two 6, of three 7 or 8): either side of the first pass's limit and
    of the probe's limit;
  * squares of 12 .. 30 border points, accepted because minMarkerPerimeterRate is low: closed inside the probe and kept by the
    rule `minPerim <= count <= maxPerim`;
  * the jagged 46-px squares, the 3-px ring with a nested frame, the one-pixel-wide ring and the spiral of
    test_gpu_parity._cell_cases, inside one cell: long outer and hole borders, pixels visited twice;
  * bars across a grid row and a grid column whose first seed state lies 38 .. 42 steps from the start (the probe keeps the start,
    the walker stops there and leaves its DevPend record) and 18 .. 22 steps from it (the probe drops the start between its 6th and
    32nd step, the border is a seed cycle);
  * two towers on a common floor, the right one four rows lower: from the starts on the right tower the first pixel in front of
    the key is ~118 forward steps away (~150 backward), so only the walker meets `pc < key`;
  * maxPerim = 26 (below the probe's 32 steps); a 40 x 36 frame.
Frames are 384 x 272 and 333 x 275 (width no multiple of the mask word), four different ones in a call of 16."""
import functools
import os

import numpy as np
import pytest

import oracle
from fiducials_amd.detector import ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary
from helpers import n_scales
from test_gpu_parity import check_stages, params_pair

SIZES = [(384, 272), (333, 275)]
DICT = 6
FRAMES = 16
MIN_RATE = 0.03  # minPerim = 0.03 * 384 = 11 (333: 9): the squares of 12 .. 30 border points pass the perimeter gate
FG, BG = 40, 215
ROADS = {"one_pass": 1, "two_passes": 2}  # FID_PROBE_PASSES
# The FID_TAP_COUNTS slot the roads may differ in: 9 = survivors of the FIRST of two passes (the single pass has none).  Slot 8, the
# point chunks that the recorded walks fill, is summed from the results and has to be the same on both roads and in every run.
ROAD_DEPENDENT_COUNTS = (9,)


def seedless_frame(w, h, variant=0):
    ox, oy = variant % 3, (variant // 3) % 3  # (every shape keeps >= 1 px from the grid lines for offsets 0 .. 2)
    img = np.full((h, w), BG, np.uint8)

    def rect(x0, y0, x1, y1, v=FG):
        img[y0 + oy:y1 + oy, x0 + ox:x1 + ox] = v

    def px(x, y, v=FG):
        img[y + oy, x + ox] = v

    # ---- cell (0, 0): small borders.  A w x h rectangle has 2 (w + h) - 4 border points, one less with a corner cut
    x = 4
    for (rw, rh, cut) in ((2, 3, 1), (2, 3, 0), (3, 3, 1), (9, 9, 1), (9, 9, 0), (9, 10, 1), (10, 9, 2), (4, 4, 0), (5, 5, 0), (6, 6, 0), (7, 7, 0),
                          (8, 8, 0), (8, 9, 0)):
        rect(x, 4, x + rw, 4 + rh)
        if cut == 1:
            px(x + rw - 1, 4 + rh - 1, BG)
        if cut == 2:
            px(x + rw - 1, 4, BG)
        x += rw + 3
    assert x < 126
    # holes of hw x hh pixels in blobs three pixels thick: 2 (hw + hh) border points, one less with a corner of the hole filled
    x, y = 4, 20
    for (hw, hh, fill) in ((1, 2, 0), (2, 2, 1), (1, 1, 0), (2, 3, 1), (7, 8, 0), (8, 8, 1), (8, 8, 0), (8, 9, 1), (8, 9, 0)):
        bw, bh = hw + 6, hh + 6
        if x + bw > 124:
            x, y = 4, y + 18
        rect(x, y, x + bw, y + bh)
        rect(x + 3, y + 3, x + 3 + hw, y + 3 + hh, BG)
        if fill:
            px(x + 3 + hw - 1, y + 3 + hh - 1)
        x += bw + 3
    assert y + 18 < 66
    # two towers on a floor, the right one four rows lower
    rect(8, 118, 61, 123)
    rect(8, 70, 19, 118)
    rect(50, 74, 61, 118)
    # ---- cell (1, 0): the long borders of _cell_cases, inside the cell
    for cx0, cy0 in ((138, 8), (200, 70)):
        rect(cx0, cy0, cx0 + 46, cy0 + 46)
        for k in range(4, 42, 4):  # notches two pixels deep on all four sides
            rect(cx0 + k, cy0, cx0 + k + 1, cy0 + 2, BG)
            rect(cx0 + k + 1, cy0 + 44, cx0 + k + 2, cy0 + 46, BG)
            rect(cx0, cy0 + k, cx0 + 2, cy0 + k + 1, BG)
            rect(cx0 + 44, cy0 + k + 1, cx0 + 46, cy0 + k + 2, BG)
    rect(196, 8, 252, 60)  # a frame 3 px wide, a nested frame inside it
    rect(199, 11, 249, 57, BG)
    rect(206, 18, 242, 50)
    rect(212, 24, 236, 44, BG)
    rect(140, 66, 141, 121)  # a one-pixel-wide ring
    rect(190, 66, 191, 121)
    rect(140, 66, 191, 67)
    rect(140, 120, 191, 121)
    # ---- cell (0, 1): the one-pixel-wide spiral
    x0, y0 = 6, 134
    for k in range(0, 56, 4):
        rect(x0 + k, y0 + k, x0 + 116 - k, y0 + k + 1)
        rect(x0 + 115 - k, y0 + k, x0 + 116 - k, y0 + 116 - k)
        rect(x0 + k + 4, y0 + 115 - k, x0 + 116 - k, y0 + 116 - k)
        rect(x0 + k + 4, y0 + k + 4, x0 + k + 5, y0 + 116 - k)
    # ---- bars across the grid row 128 and the grid column 256: first seed state 38 (+ oy / ox) and 18 steps from the start
    rect(262, 90, 276, 141)
    rect(288, 110, 302, 151)
    rect(218, 150, 271, 163)
    rect(238, 172, 281, 185)
    # ---- cell (1, 1): more small squares, a 30-px square
    for k, s in enumerate((4, 5, 6, 7, 8, 9, 10, 4, 5, 6)):
        rect(134 + 12 * (k % 5), 190 + 14 * (k // 5), 134 + 12 * (k % 5) + s, 190 + 14 * (k // 5) + s)
    rect(200, 200, 230, 230)
    return img


def tiny_frame(variant=0):
    """40 x 36: the only grid lines are row 0 and column 0."""
    img = np.full((36, 40), BG, np.uint8)
    img[3 + variant:12 + variant, 3:12] = FG  # 32 border points
    img[3:13, 16 + variant:25 + variant] = FG  # 34, minus a corner: 33
    img[12, 24 + variant] = BG
    img[18:32, 4:34] = FG  # a frame with a hole
    img[21:29, 7 + variant:31] = BG
    return img


@functools.lru_cache(maxsize=None)
def frames_of(size):
    fr = [tiny_frame(v) for v in range(4)] if size == (40, 36) else [seedless_frame(*size, v) for v in (0, 1, 4, 8)]
    for f in fr:
        f.setflags(write=False)
    return tuple(fr)


def on_grid(pts):
    return bool(np.any((pts[:, 0] % 128 == 0) | (pts[:, 1] % 128 == 0)))


@pytest.mark.parametrize("size", SIZES)
def test_the_frames_hold_what_they_were_drawn_for(size):
    """The census of the borders, by the oracle's findContours on the oracle's masks (no GPU)."""
    _, op = params_pair(minMarkerPerimeterRate=MIN_RATE)
    for img in frames_of(size):
        outer, hole, seeded = set(), set(), 0
        for s in range(n_scales(op)):
            m = oracle.adaptive_threshold(img, op.adaptiveThreshWinSizeMin + s * op.adaptiveThreshWinSizeStep, op.adaptiveThreshConstant)
            cs, holes = oracle.find_contours(m)
            for c, hl in zip(cs, holes):
                if on_grid(c):
                    seeded += 1
                else:
                    (hole if hl else outer).add(len(c))
        assert {5, 6, 7, 31, 32, 33} <= outer and {6, 7, 31, 32, 33} <= hole
        assert len(outer & set(range(12, 31))) >= 5  # closed inside the probe and accepted
        assert max(outer) > 4 * max(size) and max(hole) > 128  # the spiral runs past the perimeter cap; hole borders of more than two chunks
        assert seeded >= 4


class FrameOfBatch:
    """Frame f of a finished batch call behind the detector calls check_stages makes (it asks for frame 0 of a single call)."""

    def __init__(self, det, f, results, masks):
        self._det, self._f, self._results, self._masks = det, f, results, masks

    def detect_markers(self, gray):
        return self._results[self._f]

    def tap_masks(self, nframes, nscales, h, w):
        return self._masks[self._f:self._f + 1]

    def __getattr__(self, name):
        if name.startswith("tap_"):
            fn = getattr(self._det, name)
            return lambda *a: fn(*a)[self._f:self._f + 1]
        return getattr(self._det, name)


def stage_taps(det, frames):
    cnt = det.tap_counts()[:frames].copy()
    cand, filt, ident, pre, bits = det.tap_candidates(False), det.tap_candidates(True), det.tap_ident(), det.tap_presubpix(), det.tap_bits()
    out = []
    for f in range(frames):
        c = cnt[f]
        out.append(dict(counts=[int(v) for k, v in enumerate(c) if k not in ROAD_DEPENDENT_COUNTS], candidates=cand[f][:c[2]].tobytes(),
                        filtered=filt[f][:c[3]].tobytes(), ident=ident[f][:c[3]].tobytes(), bits=bits[f][:c[3]].tobytes(),
                        presubpix=pre[f][:c[5]].tobytes()))
    return out, cnt


ENV = ("FID_PROBE_PASSES", "FID_SEED_SHIFT")


@functools.lru_cache(maxsize=None)
def run_road(size, road, table=()):
    """One call of 16 frames on a fresh detector that takes the given road: every frame checked against the oracle, then
    (taps per frame, counters).  Computed once per (size, road, parameters) and shared."""
    saved = {k: os.environ.get(k) for k in ENV}
    os.environ.update(FID_PROBE_PASSES=str(ROADS[road]), FID_SEED_SHIFT="4")
    try:
        w, h = size
        p, op = params_pair(**dict(table or (("minMarkerPerimeterRate", MIN_RATE),)))
        d = get_predefined_dictionary(DICT)
        distinct = frames_of(size)
        batch = np.stack([distinct[f % len(distinct)] for f in range(FRAMES)])
        det = ArucoDetector(DICT, params=p, max_width=w, max_height=h, max_batch=FRAMES, max_contours=32768)
        try:
            results = det.detect_markers_batch(batch)
            masks = det.tap_masks(FRAMES, n_scales(op), h, w)
            for f in range(FRAMES):
                check_stages(FrameOfBatch(det, f, results, masks), batch[f], d, op)
            return stage_taps(det, FRAMES)
        finally:
            det.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("road", list(ROADS))
@pytest.mark.parametrize("size", SIZES)
def test_both_roads_give_the_oracles_stages(size, road):
    """What the oracle checks here and what it does not: check_stages sees candidates only behind the polygon gates, so a small
    closed border that a probe wrongly kept or dropped shows there only if it ends as a candidate; the survivor count itself
    (slot 7) is checked by the roads' comparison below, one instantiation of the probe's template against another -- not
    independent of the template, but the two-pass road stands against the oracle here as well.  The road is recognised by
    nsurv1 > nsurv, which relies on the counters being cleared for every call (the single pass never writes nsurv1)."""
    taps, cnt = run_road(size, road)
    assert all(int(c[7]) > 20 for c in cnt)  # survivors for the walker in every frame
    assert all(int(c[8]) > 0 for c in cnt)  # chunks of the frame's recorded walks (counted per frame by k_seg_cycles)
    assert all((int(c[9]) > int(c[7])) == (road == "two_passes") for c in cnt)  # (the road was taken: surv1 only behind a first pass)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_roads_agree_tap_by_tap(size):
    assert run_road(size, "one_pass")[0] == run_road(size, "two_passes")[0]


@pytest.mark.gpu
def test_a_perimeter_cap_below_the_probes_steps():
    """maxMarkerPerimeterRate 0.07: maxPerim = 26 < 32.  No start leaves the single pass undecided: the probe's own cap decides,
    as the two passes' caps did."""
    table = (("minMarkerPerimeterRate", MIN_RATE), ("maxMarkerPerimeterRate", 0.07))
    size = SIZES[0]
    assert int(0.07 * max(size)) == 26
    assert run_road(size, "one_pass", table)[0] == run_road(size, "two_passes", table)[0]


@pytest.mark.gpu
def test_a_tiny_frame():
    table = (("minMarkerPerimeterRate", 0.3),)  # minPerim 12
    size = (40, 36)
    taps, cnt = run_road(size, "one_pass", table)
    assert all(int(c[7]) >= 2 for c in cnt)
    assert taps == run_road(size, "two_passes", table)[0]
