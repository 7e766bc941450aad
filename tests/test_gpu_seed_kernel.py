"""The tracing seeds come from one of two forms of the launch sequence (FID_SEED_KERNEL): `fused` = k_find_starts<true>, which finds
starts and seeds in one loop, and `split` = k_find_starts<false> followed by k_find_seeds, a kernel that visits the seed grid's lines
only.  Both must leave the same seed SET (the list's order is undefined), so every later stage is the same: here every stage tap of
the two forms `==` each other, the candidates `==` the oracle's, and the number of seeds per frame `==` a NumPy restatement of
the seed rule (tests/test_seed_rule_restatement.py) on the oracle's threshold masks -- on the three grid spacings (FID_SEED_SHIFT
2, 3, 4: 32 / 64 / 128 px) and on frames drawn to put borders where a kernel that walks grid lines can go wrong: a pixel exactly on
a grid crossing with diagonal neighbours only, one-pixel lines and thick bars running ALONG a grid row and a grid column, checker
patches straddling grid lines (many seeds per mask word), shapes on the image's first and last row and column; sizes whose last
row and column are grid lines themselves (257 x 257: the grid column's mask word holds ONE pixel), whose width is no multiple of
the mask word (333 x 275), and 384 x 272."""
import functools
import re

import numpy as np
import pytest

import oracle
from fiducials_amd.detector import ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary
from helpers import n_scales
from test_gpu_chain_codes import check_candidates
from test_gpu_parity import params_pair
from test_seed_rule_restatement import seed_count

pytestmark = pytest.mark.gpu

SIZES = [(257, 257), (333, 275), (384, 272)]
FORMS = ("split", "fused")
DICT = 6


def grid_frame(w, h, variant=0):
    """Dark shapes on a light ground, placed by the 128-px grid (whose lines are lines of the 32- and 64-px grids too)."""
    rng = np.random.default_rng(100 * w + h + variant)
    img = np.full((h, w), 215, np.uint8)
    fg = 40
    # a square ring that crosses grid lines on all four sides: a quad for the candidate stages
    img[70 + variant:190, 60:200 - variant] = fg
    img[86 + variant:174, 76:184 - variant] = 215
    # a pixel exactly on the crossing (128, 128) with diagonal neighbours only
    for dx, dy in ((0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1), (2, 2), (-2, 2)):
        img[128 + dy, 128 + dx] = fg
    # one-pixel lines and thick bars along a grid row and along a grid column (on the line, and the bar's edge on the line)
    img[128, 8:56] = fg
    img[10:60, 128] = fg
    img[192:200, 20:110] = fg   # (rows 192 .. 199: its first row is a line of the 64-px grid)
    img[200:250, 121:129] = fg  # (columns 121 .. 128: its last column is the grid column)
    if w > 300:
        img[122:135, 262:320] = fg  # thick bar with the grid row 128 inside it
        img[20:100, 250:263] = fg   # thick bar with the grid column 256 inside it
    # checker patches straddling grid lines: one-pixel cells (every bit of a word) and three-pixel cells
    yy, xx = np.mgrid[0:h, 0:w]
    patch = (xx >= 206) & (xx < 250) & (yy >= 110) & (yy < 146)
    img[patch & ((xx + yy) % 2 == 0)] = fg
    patch = (xx >= 100) & (xx < 160) & (yy >= 20) & (yy < 44) & (xx != 128)
    img[patch & (((xx // 3) + (yy // 3)) % 2 == 0)] = fg
    # shapes touching the image's first and last row and column
    img[0:9, 0:14] = fg
    img[0, 30:90] = fg
    img[h - 7:h, w - 12:w] = fg
    img[h - 1, 10:70] = fg
    img[60:120, 0] = fg
    img[150:230, w - 1] = fg
    img[h - 30:h, 40:52] = fg
    img[0:25, w - 40:w - 28] = fg
    # a few ragged blobs
    for _ in range(6):
        x0, y0 = int(rng.integers(0, w - 20)), int(rng.integers(0, h - 20))
        blob = rng.random((14, 18)) < 0.55
        sub = img[y0:y0 + 14, x0:x0 + 18]
        sub[blob[:sub.shape[0], :sub.shape[1]]] = fg
    return img


@functools.lru_cache(maxsize=None)
def reference(w, h, variant=0, table=None):
    """(frame, oracle trace, seed counts by grid spacing) -- computed once, shared, never changed."""
    img = grid_frame(w, h, variant)
    img.setflags(write=False)
    _, op = params_pair(**(dict(table) if table else {}))
    _, _, tr = oracle.detect(img, get_predefined_dictionary(DICT), params=op, trace=True)
    masks = [oracle.adaptive_threshold(img, op.adaptiveThreshWinSizeMin + s * op.adaptiveThreshWinSizeStep, op.adaptiveThreshConstant)
             for s in range(n_scales(op))]
    seeds = {g: sum(seed_count(m, g) for m in masks) for g in (32, 64, 128)}
    return img, tr, seeds


def taps(det, frames):
    """Every stage tap of the last call, cut to what each frame's counters say is filled."""
    cnt = det.tap_counts()[:frames].copy()
    cand, filt, ident, pre = det.tap_candidates(False), det.tap_candidates(True), det.tap_ident(), det.tap_presubpix()
    out = []
    for f in range(frames):
        c = cnt[f]
        out.append(dict(counts=c.tolist(), candidates=cand[f][:c[2]].tobytes(), filtered=filt[f][:c[3]].tobytes(),
                        ident=ident[f][:c[3]].tobytes(), presubpix=pre[f][:c[5]].tobytes()))
    return out


def run_form(monkeypatch, form, shift, frames, params=None, **kw):
    """One call on a fresh detector of the given form: (taps per frame, candidates per frame, counters, results)."""
    monkeypatch.setenv("FID_SEED_KERNEL", form)
    if shift:
        monkeypatch.setenv("FID_SEED_SHIFT", str(shift))
    else:
        monkeypatch.delenv("FID_SEED_SHIFT", raising=False)
    h, w = frames[0].shape
    det = ArucoDetector(DICT, params=params, max_width=w, max_height=h, max_batch=len(frames), **kw)
    try:
        res = [det.detect_markers(frames[0])] if len(frames) == 1 else det.detect_markers_batch(np.stack(frames))
        cnt = det.tap_counts()[:len(frames)].copy()
        cands = [det.tap_candidates(False)[f][:cnt[f][2]].copy() for f in range(len(frames))]
        return taps(det, len(frames)), cands, cnt, res
    finally:
        det.close()


@pytest.mark.parametrize("shift", [2, 3, 4])
@pytest.mark.parametrize("size", SIZES)
def test_both_forms_on_grid_line_frames(monkeypatch, size, shift):
    img, tr, seeds = reference(*size)
    assert seeds[8 << shift] > 50  # (the frame does what it was drawn for)
    got = {form: run_form(monkeypatch, form, shift, [img]) for form in FORMS}
    for form in FORMS:
        _, cands, cnt, _ = got[form]
        check_candidates(cands[0], cnt[0], tr)
        assert cnt[0][10] == seeds[8 << shift], f"{form}: seeds on the {8 << shift}-px grid"
    assert got["split"][0] == got["fused"][0]


def test_three_different_frames_in_one_call(monkeypatch):
    w, h = 333, 275
    refs = [reference(w, h, v) for v in (0, 3, 6)]
    assert len({r[0].tobytes() for r in refs}) == 3
    got = {form: run_form(monkeypatch, form, 4, [r[0] for r in refs]) for form in FORMS}
    for form in FORMS:
        _, cands, cnt, _ = got[form]
        for f, (_, tr, seeds) in enumerate(refs):
            check_candidates(cands[f], cnt[f], tr)
            assert cnt[f][10] == seeds[128]
    assert got["split"][0] == got["fused"][0]


def test_a_batch_cut_into_two_sub_batches(monkeypatch):
    """32 frames: two sub-batches on their own streams, each with its own k_find_seeds; the grid spacing
    and the form are the defaults of a batch (128 px, split) -- and forced `fused` beside it."""
    w, h = 257, 257
    refs = [reference(w, h, v) for v in (0, 3, 6)]
    frames = [refs[f % 3][0] for f in range(32)]
    monkeypatch.delenv("FID_SEED_KERNEL", raising=False)
    monkeypatch.delenv("FID_SEED_SHIFT", raising=False)
    det = ArucoDetector(DICT, max_width=w, max_height=h, max_batch=32)
    try:
        det.detect_markers_batch(np.stack(frames))
        default = taps(det, 32)
        cnt = det.tap_counts()[:32].copy()
        for f in (0, 1, 2, 19, 20, 21, 31):
            check_candidates(det.tap_candidates(False)[f][:cnt[f][2]], cnt[f], refs[f % 3][1])
        assert [int(c[10]) for c in cnt] == [refs[f % 3][2][128] for f in range(32)]
    finally:
        det.close()
    for form in FORMS:
        assert run_form(monkeypatch, form, 0, frames)[0] == default


def test_two_scale_threshold_table(monkeypatch):
    """nscales != 13: the kernel takes the number of mask planes from the call's parameters."""
    table = (("adaptiveThreshWinSizeMin", 5), ("adaptiveThreshWinSizeMax", 13), ("adaptiveThreshWinSizeStep", 8))
    img, tr, seeds = reference(384, 272, 0, table)
    p, op = params_pair(**dict(table))
    assert n_scales(op) == 2 and seeds[128] > 10
    got = {form: run_form(monkeypatch, form, 4, [img], params=p) for form in FORMS}
    for form in FORMS:
        _, cands, cnt, _ = got[form]
        check_candidates(cands[0], cnt[0], tr)
        assert cnt[0][10] == seeds[128]
    assert got["split"][0] == got["fused"][0]


def comb_frame():
    """384 x 272, noisy, with combs whose one-pixel teeth cross the lines of the 128-px grid: a handful of borders with thousands of
    seed states -- far more seeds than border-following starts that survive the probes."""
    from fiducials_amd.synth import make_frame

    w, h = 384, 272
    img = make_frame(get_predefined_dictionary(DICT), 9, width=w, height=h, n_markers=2, side_range=(44, 60)).image.copy()
    rng = np.random.default_rng(5)
    for y in (128, 256):  # spines above the grid rows, teeth down across them
        img[y - 10:y - 7, 4:w - 4] = 30
        img[y - 10:y + 8, 4:w - 4:2] = 30
        img[y - 10:y + 8, 5:w - 4:2] = 220
        img[y - 10:y - 7, 4:w - 4] = 30
    for x in (128, 256):  # spines left of the grid columns, teeth across them
        img[4:h - 4:2, x - 10:x + 8] = 30
        img[5:h - 4:2, x - 10:x + 8] = 220
        img[4:h - 4, x - 10:x - 7] = 30
    salt = rng.random((h, w)) < 0.01
    img[salt] = rng.integers(0, 256, int(salt.sum()))
    return img


def test_seed_table_overflow_in_both_forms(monkeypatch, capfd):
    """A seed table far too small for the frame: both forms clip their writes, raise the contour-table flag (bit 1 of the global
    overflow word, printed by FID_VERBOSE when the call falls back), and the call's answer through the whole-border walk is the
    oracle's."""
    img = comb_frame()
    d = get_predefined_dictionary(DICT)
    oids, ocorners = oracle.detect(img, d)
    op = oracle.default_params()
    nseeds = sum(seed_count(oracle.adaptive_threshold(img, op.adaptiveThreshWinSizeMin + s * op.adaptiveThreshWinSizeStep,
                                                      op.adaptiveThreshConstant), 128) for s in range(n_scales(op)))
    cap = 2048
    assert nseeds > 4 * cap and len(oids) >= 1
    monkeypatch.setenv("FID_VERBOSE", "1")
    for form in FORMS:
        capfd.readouterr()
        _, _, cnt, res = run_form(monkeypatch, form, 4, [img], max_contours=cap)
        err = capfd.readouterr().err
        m = re.search(r"seed tracing overflow flags 0x([0-9a-f]+) \(frame 0: seeds (\d+)", err)
        assert m, f"{form}: the call did not fall back: {err!r}"
        assert int(m.group(1), 16) & 2, form
        assert int(m.group(2)) == nseeds, form  # (the counter counts every seed, written or not)
        corners, ids = res[0]
        assert ids.tolist() == oids.tolist() and np.array_equal(corners, ocorners), form
