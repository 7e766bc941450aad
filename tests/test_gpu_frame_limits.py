"""The aruco path at the edges of what fid_detect accepts: frames of 8 .. 8191 px a side, threshold windows up to 2 * 8191 + 1 px,
32 threshold scales, and one batch of more than 2^31 bytes of gray.  Every threshold mask is compared with the int64 reference
(helpers.adaptive_threshold_ref) up to 4096^2 px and with the oracle above, and the tables are chosen so that each K1 kernel runs
at its edge shapes: the node's default table goes to k_threshold_stream, tables with rmax <= 40 to k_threshold, wider ones to
k_threshold_wide.  Run on the MI355X: -m gpu."""
import numpy as np
import pytest

import oracle
from fiducials_amd import _lib
from fiducials_amd._lib import FidError
from fiducials_amd.detector import ArucoDetector
from fiducials_amd.dictionary import draw_marker, get_predefined_dictionary
from fiducials_amd.synth import make_frame
from helpers import adaptive_threshold_ref, n_scales
from test_gpu_parity import check_stages, params_pair

pytestmark = pytest.mark.gpu

D4 = get_predefined_dictionary("DICT_4X4_50")


def _table(t):
    return dict(adaptiveThreshWinSizeMin=t[0], adaptiveThreshWinSizeMax=t[1], adaptiveThreshWinSizeStep=t[2])


def _windows(p):
    return [p.adaptiveThreshWinSizeMin + s * p.adaptiveThreshWinSizeStep for s in range(n_scales(p))]


def _same(a, b):
    assert a[1].tolist() == b[1].tolist()
    assert np.array_equal(a[0], b[0])


def _thr_frame(w, h, kind, seed):
    """Frames for the mask tests: 255 with a dark square (the largest box sums), noise, half-bright noise, noisy ramps."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        g = np.full((h, w), 255, np.uint8)
        g[h // 4:h // 4 + max(h // 2, 1), w // 4:w // 4 + max(w // 2, 1)] = 200
        return g
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == 1:
        return noise
    if kind == 2:
        noise[:, w // 2:] = 250
        return noise
    ramp = np.add.outer(np.arange(h) * 97 // h, np.arange(w) * 151 // w)
    return np.clip(ramp + rng.integers(-12, 13, (h, w)), 0, 255).astype(np.uint8)


def _thr_stack(w, h, n, seed):
    return np.stack([_thr_frame(w, h, i % 4, seed + i) for i in range(n)])


def _check_masks(det, frames, p, against="ref"):
    """The threshold masks of every frame of the last call and every scale == the int64 reference (or the oracle)."""
    n, h, w = frames.shape
    masks = det.tap_masks(n, n_scales(p), h, w)
    for f in range(n):
        for s, win in enumerate(_windows(p)):
            if against == "ref":
                want = adaptive_threshold_ref(frames[f], win, p.adaptiveThreshConstant) > 0
            else:
                want = oracle.adaptive_threshold(frames[f], win, p.adaptiveThreshConstant) > 0
            got = masks[f, s] > 0
            assert np.array_equal(got, want), f"{w}x{h} frame {f} scale {s} (win {win}): {(got != want).sum()} px differ"


def _batch_case(det, frames):
    """Batches of 1, 3 and F frames: every mask == the reference, and frame f of the batch == a single call on frame f."""
    p = det.params
    single = []
    for f in range(len(frames)):
        single.append(det.detect_markers(frames[f]))
        _check_masks(det, frames[f:f + 1], p)
    for n in sorted({1, 3, len(frames)}):
        if n > len(frames):
            continue
        got = det.detect_markers_batch(frames[:n])
        _check_masks(det, frames[:n], p)
        for f in range(n):
            _same(got[f], single[f])


# ---- K1 kernels at their edge shapes ---------------------------------------------------------------------------------------

STREAM_W = [8, 9, 63, 64, 65, 191, 192, 193, 319, 320, 321, 385]  # around strips of 64 * NW columns (NW = 3 and 5)
STREAM_H = [8, 9, 15, 16, 17, 63, 65]


def _is_node_table(p):
    return n_scales(p) == 13 and _windows(p) == [3 + 4 * i for i in range(13)]


@pytest.fixture(scope="module")
def node_det():
    det = ArucoDetector(D4, max_width=385, max_height=65, max_batch=8)
    assert _is_node_table(det.params)  # (k_threshold_stream)
    yield det
    det.close()


@pytest.mark.parametrize("w", STREAM_W)
def test_stream_kernel_frame_sizes(node_det, w):
    """k_threshold_stream: every height at this width, in batches of 1, 3 and 8 (its row segments depend on the batch size)."""
    for h in STREAM_H:
        _batch_case(node_det, _thr_stack(w, h, 8, 100 * w + h))


STREAM_VARIANTS = [{"FID_THR_NW": "5"}, {"FID_THR_SPLIT": "1"}, {"FID_THR_NW": "5", "FID_THR_SPLIT": "1"}, {"FID_THR_XCD": "0"},
                   {"FID_THR_ROWS": "4"}, {"FID_THR_ROWS": "12"}]


@pytest.mark.parametrize("env", STREAM_VARIANTS, ids=[",".join(f"{k}={v}" for k, v in e.items()) for e in STREAM_VARIANTS])
def test_stream_kernel_variants(monkeypatch, env):
    """The k_threshold_stream variants fid_create reads from the environment, on a subset of the shapes."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    det = ArucoDetector(D4, max_width=385, max_height=65, max_batch=8)
    try:
        for w in (8, 65, 193, 321, 385):
            for h in (9, 17, 65):
                _batch_case(det, _thr_stack(w, h, 8, 7000 + 100 * w + h))
    finally:
        det.close()


SMALL_SHAPES = [(8, 8), (9, 63), (65, 17), (193, 65), (385, 9)]  # (width, height)
# (min, max, step); the last has 32 scales (FID_MAX_SCALES), so the scale index reaches 31
TILE_TABLES = [(81, 81, 1), (5, 45, 8), (3, 65, 2)]


@pytest.mark.parametrize("table", TILE_TABLES, ids=[f"{a}-{b}-{c}" for a, b, c in TILE_TABLES])
def test_tile_kernel_tables(table):
    """k_threshold (rmax <= 40): windows up to 81, and a table of 32 scales."""
    p, _ = params_pair(**_table(table))
    assert max(_windows(p)) <= 81 and not _is_node_table(p)
    if table == (3, 65, 2):
        assert n_scales(p) == 32
    det = ArucoDetector(D4, params=p, max_width=385, max_height=65, max_batch=3)
    try:
        for w, h in SMALL_SHAPES:
            _batch_case(det, _thr_stack(w, h, 3, 300 * w + h))
    finally:
        det.close()


# windows above 81 px: around the oracle's old int32 limit (2049 / 2051), above 2^23 px of area (2897), the widest (16383)
WIDE_TABLES = [(83, 83, 1), (2049, 2049, 1), (2051, 2051, 1), (2053, 2053, 1), (2899, 2899, 1), (16383, 16383, 1), (3, 16383, 8190),
               (3, 251, 8)]


@pytest.mark.parametrize("table", WIDE_TABLES, ids=[f"{a}-{b}-{c}" for a, b, c in WIDE_TABLES])
def test_wide_kernel_tables(table):
    """k_threshold_wide (rmax > 40) on small frames, where the window is many times wider and taller than the frame."""
    p, _ = params_pair(**_table(table))
    assert max(_windows(p)) > 81
    if table == (3, 251, 8):
        assert n_scales(p) == 32
    det = ArucoDetector(D4, params=p, max_width=385, max_height=65, max_batch=3)
    try:
        for w, h in SMALL_SHAPES:
            _batch_case(det, _thr_stack(w, h, 3, 500 * w + h))
    finally:
        det.close()


@pytest.mark.parametrize("table", [(83, 2053, 1970), (16383, 16383, 1), (3, 16383, 8190), (3, 251, 8)],
                         ids=["83-2053", "16383", "3-16383-8190", "3-251-8"])
def test_wide_kernel_8191_px_rows(table):
    """k_threshold_wide on 8191-px rows: 16 columns a thread (K = WT) and (W + 9) * 8 bytes of LDS, past 64 KiB."""
    p, _ = params_pair(**_table(table))
    det = ArucoDetector(D4, params=p, max_width=8191, max_height=40, max_batch=3, max_starts=1 << 22, max_contours=1 << 17,
                       max_points=1 << 26)  # (32 scales of noise)
    try:
        for h in (8, 40):
            _batch_case(det, _thr_stack(8191, h, 3, 900 + h))
    finally:
        det.close()


# ---- the whole pipeline at the frame extremes ------------------------------------------------------------------------------

def _canvas(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = 120 + 30 * np.sin(3 * xx / w + 2 * yy / h) + rng.normal(0, 2, (h, w)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def _paste(img, marker_id, x, y, side, quiet):
    """dictionary.draw_marker at (x, y) in a white quiet zone of `quiet` px (clipped by the frame's edges)."""
    img[max(y - quiet, 0):y + side + quiet, max(x - quiet, 0):x + side + quiet] = 255
    img[y:y + side, x:x + side] = draw_marker(D4, marker_id, side)


def _pipeline_case(w, h, img, drawn, table=None, limits=None, **kw):
    """check_stages (every stage == the oracle, corners bit for bit; no capacity flag) and the drawn ids found."""
    p, op = params_pair(**(_table(table) if table else {}), **kw)
    det = ArucoDetector(D4, params=p, max_width=w, max_height=h, **(limits or {}))
    try:
        _, ids, _ = check_stages(det, img, D4, op)
        assert det.tap_counts()[0][6] == 0
        assert sorted(ids.tolist()) == sorted(drawn)
        return det.tap_candidates(False)[0][:det.tap_counts()[0][2]]
    finally:
        det.close()


def test_smallest_frames():
    """8 x 8 and 16 x 16 with a 4x4 marker at 1 px per cell, 16 x 16 with one at 2 px per cell."""
    img = _canvas(8, 8, 1)
    _paste(img, 3, 1, 1, 6, 1)
    _pipeline_case(8, 8, img, [3], minDistanceToBorder=1)
    img = _canvas(16, 16, 2)
    _paste(img, 5, 5, 5, 6, 5)
    _pipeline_case(16, 16, img, [5])
    img = _canvas(16, 16, 3)
    _paste(img, 7, 2, 2, 12, 2)
    _pipeline_case(16, 16, img, [7], minDistanceToBorder=1)


@pytest.mark.parametrize("size", [(8, 8191), (8191, 8)], ids=["8x8191", "8191x8"])
def test_thin_frames(size):
    """A column and a row of 8191 px, with dark blobs along them."""
    w, h = size
    img = _canvas(w, h, 4)
    for k in range(40, 8100, 700):
        if w == 8:
            img[k:k + 200, 2:6] = 20
        else:
            img[2:6, k:k + 200] = 20
    _pipeline_case(w, h, img, [])


@pytest.fixture(scope="module")
def frames_4k():
    return [make_frame(D4, 6100 + i, width=3840, height=2160, n_markers=20, side_range=(180, 420)) for i in range(4)]


def test_4k_frame(frames_4k):
    """3840 x 2160: every stage == the oracle, and every threshold mask == the int64 reference."""
    fr = frames_4k[0]
    det = ArucoDetector(D4, max_width=3840, max_height=2160)
    try:
        _, ids, _ = check_stages(det, fr.image, D4)
        assert sorted(ids.tolist()) == sorted(fr.ids.tolist())
        _check_masks(det, fr.image[None], det.params)
    finally:
        det.close()


def test_4k_batch(frames_4k):
    """3840 x 2160 at F = 4: frame f of the batch == a single call on frame f == the oracle."""
    frames = np.stack([fr.image for fr in frames_4k])
    det = ArucoDetector(D4, max_width=3840, max_height=2160, max_batch=4)
    try:
        batch = det.detect_markers_batch(frames)
        assert (det.tap_counts()[:, 6] == 0).all()
        for f, fr in enumerate(frames_4k):
            single = det.detect_markers(frames[f])
            oids, ocorners = oracle.detect(frames[f], D4)
            _same(batch[f], single)
            _same(single, (ocorners, oids))
            assert sorted(oids.tolist()) == sorted(fr.ids.tolist())
    finally:
        det.close()


def test_8191_corners_past_4096_and_at_the_edges():
    """Markers whose corners lie at x, y >= 4096 (the top bit of 13-bit packed coordinates) and 4 px from the right and bottom
    edges."""
    n, side = 8191, 240
    img = _canvas(n, n, 5)
    e = n - side - 4  # the last corner at 8186: 4 px from the edge, minDistanceToBorder = 3
    spots = [(4100, 4100), (e, e), (e, 4400), (4400, e), (6000, 7000), (7300, 5200), (200, e), (e, 300)]
    for i, (x, y) in enumerate(spots):
        _paste(img, 10 + i, x, y, side, 40)
    cands = _pipeline_case(n, n, img, [10 + i for i in range(len(spots))])
    assert cands["corners"].max() > n - 6


def test_8191_one_marker_of_7000_px():
    """One marker about 7000 px a side: its border contours are about 28 000 points, close to maxPerim = 4 * 8191."""
    n, side = 8191, 7002
    img = _canvas(n, n, 6)
    _paste(img, 21, 590, 590, side, 300)
    cands = _pipeline_case(n, n, img, [21])
    assert cands["contour_size"].max() >= 27000


def test_8191_widest_windows():
    """8191 x 8191 with the (3, 16383, 8190) table: windows 3, 8193 and 16383 (k_threshold_wide), masks == the oracle."""
    n = 8191
    img = _canvas(n, n, 7)
    spots = [(1000, 1000), (5000, 2000), (3000, 6500), (7000, 7000)]
    for i, (x, y) in enumerate(spots):
        _paste(img, 30 + i, x, y, 600, 100)
    # (at 8193 and 16383 px the mean is nearly the frame's: the dark half of the background is foreground, with a noisy edge)
    _pipeline_case(n, n, img, [30 + i for i in range(len(spots))], table=(3, 16383, 8190),
                   limits=dict(max_starts=1 << 22, max_contours=1 << 18, max_points=1 << 26))


def test_frame_size_refusals():
    """Width or height 7 or 8192 is refused with FID_E_INVALID_ARG (8192 even where the context was made for it); 8 and 8191
    are accepted."""
    det = ArucoDetector(D4, max_width=8192, max_height=8192)
    try:
        for w, h in ((7, 8), (8, 7), (8192, 8), (8, 8192)):
            with pytest.raises(FidError) as e:
                det.detect_markers(np.full((h, w), 128, np.uint8))
            assert e.value.status == _lib.FID_E_INVALID_ARG, (w, h)
        for w, h in ((8, 8), (8191, 8), (8, 8191)):
            det.detect_markers(np.full((h, w), 128, np.uint8))
    finally:
        det.close()


# ---- one batch of more than 2^31 bytes -------------------------------------------------------------------------------------

def test_batch_past_2_31_bytes():
    """F = 1040 frames of 1920 x 1080 resident on the device (2.157e9 px: the last frames start beyond 2^31), as mono8 (gray
    aliases the caller's buffer) and as bgr8 (k_to_gray writes the context's own F * W * H buffer): every frame == a single call on
    its base frame == the oracle, and no frame overflows the reduced limits."""
    import torch

    F, W, H = 1040, 1920, 1080
    assert (F - 1) * W * H > 2 ** 31
    base = [make_frame(D4, 6500 + i, n_markers=16, side_range=(100, 170)) for i in range(8)]
    gray = np.stack([fr.image for fr in base])
    free0 = torch.cuda.mem_get_info()[0]
    det = ArucoDetector(D4, max_width=W, max_height=H, max_batch=F, max_starts=131072, max_contours=8192, max_points=2 << 20,
                        max_candidates=1024)
    dev = None
    try:
        want = []
        for f in range(8):
            single = det.detect_markers(gray[f])
            oids, ocorners = oracle.detect(gray[f], D4)
            _same(single, (ocorners, oids))
            assert sorted(oids.tolist()) == sorted(base[f].ids.tolist())
            want.append(single)
        idx = torch.arange(F, device="cuda") % 8
        for enc in ("mono8", "bgr8"):
            src = torch.from_numpy(gray).cuda()
            if enc == "bgr8":
                src = src[..., None].expand(8, H, W, 3).contiguous()  # (B = G = R: BGR2GRAY gives the gray back)
            dev = src[idx].contiguous()
            del src
            torch.cuda.synchronize()
            got = det.detect_markers_device(dev.data_ptr(), F, W, H, encoding=enc)
            used = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 30
            print(f"\n{enc}: {F} frames, input {dev.numel() / 2 ** 30:.2f} GiB, device memory in use (context + input) {used:.2f} GiB")
            cnt = det.tap_counts()
            assert cnt.shape[0] == F and (cnt[:, 6] == 0).all(), np.flatnonzero(cnt[:, 6])
            for f in range(F):
                _same(got[f], want[f % 8])
            del dev
            dev = None
            torch.cuda.empty_cache()
    finally:
        det.close()
        del dev
        torch.cuda.empty_cache()
