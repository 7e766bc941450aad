"""STag on frames that are already in device memory (fid_stag_detect_markers_device / fid_stag_detect_markers_batch_device,
k_stag_ingest): a torch tensor, a padded pitch, colour frames, a decoded JPEG batch.  Every result must be byte-identical to the
host road (fid_stag_detect_markers / _batch) on the same gray image; colour goes to gray in OpenCV 4.x's 15-bit form."""
import ctypes as C
import io
import re

import numpy as np
import pytest

from fiducials_amd import _lib, synth
from fiducials_amd import stag as fstag
from fiducials_amd._lib import FidError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K720 = np.array([[933.3, 0, 640.0], [0, 933.3, 360.0], [0, 0, 1]])


def gray15(bgr):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15).astype(np.uint8)


def gray14(bgr):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def divergent_triples():
    """every (B, G, R) where the 15-bit and the 14-bit fixed-point gray differ: (n, 3) uint8, B G R"""
    v = np.arange(1 << 24, dtype=np.int64)
    bgr = np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1)
    d = gray15(bgr) != gray14(bgr)
    return bgr[d].astype(np.uint8)


def tinted(gray, seed):
    """a colour frame whose channels differ (so its gray is not the input) with the marker contrast kept"""
    rng = np.random.default_rng(seed)
    g = gray.astype(np.int64)
    b = np.clip(g * 0.85 + 20 + rng.integers(-6, 7, g.shape), 0, 255)
    r = np.clip(g * 1.1 - 8 + rng.integers(-6, 7, g.shape), 0, 255)
    gg = np.clip(g + rng.integers(-3, 4, g.shape), 0, 255)
    return np.stack([b, gg, r], axis=-1).astype(np.uint8)


def to_device(arr, pitch=None, offset=0, fill=0xA5):
    """arr (H, W[, C]) uint8 -> a cuda uint8 tensor holding its rows `pitch` bytes apart, starting `offset` bytes in (the padding
    holds `fill`: a kernel that read it would show).  -> (tensor, pointer of row 0, pitch)"""
    h = arr.shape[0]
    row = arr.reshape(h, -1)
    pitch = pitch or row.shape[1]
    buf = np.full(offset + h * pitch + 64, fill, np.uint8)
    view = buf[offset:offset + h * pitch].reshape(h, pitch)
    view[:, :row.shape[1]] = row
    t = torch.from_numpy(buf).to("cuda")
    torch.cuda.synchronize()
    return t, t.data_ptr() + offset, pitch


def host_result(det, gray, K=K720):
    m = det.detect_markers(gray)
    return m.tobytes(), det.pose_last(K, None, 0.18).tobytes(), len(m)


def device_result(det, ptr, w, h, pitch, enc, K=K720):
    m = det.detect_markers_device(ptr, w, h, pitch, enc)
    return m.tobytes(), det.pose_last(K, None, 0.18).tobytes(), len(m)


@pytest.mark.parametrize("size,pitch,offset,markers", [((1920, 1080), None, 0, True), ((1920, 1080), 2048, 0, True),
                                                       ((1280, 720), 1283, 7, True), ((1917, 1079), 1920, 3, True),
                                                       ((333, 127), None, 0, False), ((333, 127), 351, 5, False)])
def test_mono8_from_a_torch_tensor_equals_the_host_road(size, pitch, offset, markers):
    w, h = size
    words = fstag.load_library(21)
    n = 12 if w >= 1280 else 2
    side = (110.0, 200.0) if w >= 1280 else (40.0, 55.0)
    gray = synth.make_stag_frame(words, 700 + w + h, w, h, n, side_range=side).image
    t, ptr, p = to_device(gray, pitch, offset)
    K = synth.K_DEFAULT if w >= 1900 else K720
    host = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    dev = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        want = host_result(host, gray, K)
        got = device_result(dev, ptr, w, h, p, "mono8", K)
        assert got == want
        if markers:
            assert want[2] >= 3
        for tap in (fstag.TAP_GRAY, fstag.TAP_SMOOTH, fstag.TAP_GRAD):
            assert dev.tap(tap).tobytes() == host.tap(tap).tobytes(), tap
        assert np.array_equal(dev.tap(fstag.TAP_GRAY), gray)
        assert np.array_equal(host.tap(fstag.TAP_GRAY), gray)  # (the tap after a host call: what was staged)
    finally:
        host.close()
        dev.close()
    del t


@pytest.mark.parametrize("enc,pitch,offset", [("bgr8", None, 0), ("rgb8", None, 0), ("bgr8", 3 * 1920 + 16, 0), ("rgb8", 3 * 1920 + 5, 1)])
def test_colour_frames_go_to_gray_in_the_15_bit_form(enc, pitch, offset):
    """cvtColor's RGB2Gray<uchar> in OpenCV 4.x's 15-bit form, exactly -- including every one of the 43 864 colours on which the
    14-bit form (StagNode::msgToGray) gives another value -- and then the host road's markers and poses on that gray."""
    w, h = 1920, 1080
    words = fstag.load_library(21)
    bgr = tinted(synth.make_stag_frame(words, 811, w, h, 12).image, 3)
    div = divergent_triples()
    assert len(div) == 43864
    rows = -(-len(div) // w)
    block = np.resize(div, (rows * w, 3)).reshape(rows, w, 3)
    bgr[h - rows:] = block  # (the bottom rows: every divergent colour at least once)
    src = bgr if enc == "bgr8" else np.ascontiguousarray(bgr[..., ::-1])
    want_gray = gray15(bgr)
    assert (want_gray != gray14(bgr)).sum() >= 43864
    t, ptr, p = to_device(src, pitch, offset)
    host = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    dev = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    try:
        got = device_result(dev, ptr, w, h, p, enc, synth.K_DEFAULT)
        assert np.array_equal(dev.tap(fstag.TAP_GRAY), want_gray)
        want = host_result(host, want_gray, synth.K_DEFAULT)
        assert want[2] >= 3 and got == want
        assert dev.tap(fstag.TAP_SMOOTH).tobytes() == host.tap(fstag.TAP_SMOOTH).tobytes()
    finally:
        host.close()
        dev.close()
    del t


def _frames(words, w, h, n, seed, n_markers=6):
    return [synth.make_stag_frame(words, seed + i, w, h, n_markers, side_range=(70.0, 120.0)).image for i in range(n)]


@pytest.mark.parametrize("nctx,nframes,enc,spec", [(4, 7, "mono8", None), (4, 7, "bgr8", "1"), (64, 70, "mono8", "1"), (64, 70, "bgr8", None)])
def test_device_batch_equals_the_frame_at_a_time_road(nctx, nframes, enc, spec, monkeypatch, capfd):
    """Frame counts that are not a multiple of the group size (groups of 2 on 4 slots, of 32 on 64), frames a padded frame stride
    apart, on the counted road and queued ahead (FID_STAG_SPEC=1): every frame == fid_stag_detect_markers + fid_stag_pose_last on
    one context.  The ingest of a group is one launch: on the counted road no frame's arguments fail to fit the launch open at its
    site (FID_VERBOSE's count)."""
    w, h = 640, 480
    K = np.array([[466.7, 0, 320.0], [0, 466.7, 240.0], [0, 0, 1]])
    words = fstag.load_library(21)
    uniq = _frames(words, w, h, 5, 900)
    grays = [uniq[(3 * i) % len(uniq)] for i in range(nframes)]
    if enc == "bgr8":
        colour = [tinted(g, i) for i, g in enumerate(uniq)]
        src = [colour[(3 * i) % len(uniq)] for i in range(nframes)]
        grays = [gray15(c) for c in src]
        bpp = 3
    else:
        src, bpp = grays, 1
    pitch = w * bpp + 32
    fstride = pitch * h + 4096 + 48
    buf = np.full(nframes * fstride, 0x3C, np.uint8)
    for f, s in enumerate(src):
        buf[f * fstride:f * fstride + pitch * h].reshape(h, pitch)[:, :w * bpp] = s.reshape(h, -1)
    t = torch.from_numpy(buf).to("cuda")
    torch.cuda.synchronize()
    one = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    try:
        want = [host_result(one, g, K) for g in grays]
    finally:
        one.close()
    assert all(x[2] >= 3 for x in want)
    if spec:
        monkeypatch.setenv("FID_STAG_SPEC", spec)
    monkeypatch.setenv("FID_VERBOSE", "1")
    pool = fstag.StagPool(21, 7, n_contexts=nctx, max_width=w, max_height=h)
    try:
        capfd.readouterr()
        for rnd in range(2):  # (the second call: slots that remember their last frame -- queued ahead with FID_STAG_SPEC=1)
            M, P = pool.detect_markers_batch_device(t.data_ptr(), nframes, w, h, pitch, fstride, enc, K, None, 0.18)
            assert len(M) == nframes
            for f in range(nframes):
                assert (M[f].tobytes(), P[f].tobytes(), len(M[f])) == want[f], (rnd, f)
        err = capfd.readouterr().err
        unfit = re.findall(r"\((\d+) times a frame's arguments did not fit", err)
        assert len(unfit) == 2, err[-2000:]
        if not spec:  # (queued ahead, frames whose predicted sizes differ launch apart at the sized sites, host frames alike)
            assert unfit == ["0", "0"], err[-2000:]
        if spec:
            assert sum(d.queue_stats()[0] for d in pool.dets) > 0
    finally:
        pool.close()
    del t


def test_ten_device_frames_on_one_context_are_queued_ahead_and_still_match():
    words = fstag.load_library(21)
    w, h = 1280, 720
    small = _frames(words, w, h, 2, 950, 3)
    big = _frames(words, w, h, 2, 960, 10)
    seq = [small[0], small[1], small[0], big[0], big[1], big[0], small[0], big[1], small[1], small[1]]
    host = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    dev = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    try:
        want = [host_result(host, g) for g in seq]
        assert sum(x[2] >= 3 for x in want) >= 8
        stack = np.stack(seq)
        t = torch.from_numpy(stack).to("cuda")
        torch.cuda.synchronize()
        for k in range(len(seq)):
            assert device_result(dev, t.data_ptr() + k * w * h, w, h, w, "mono8") == want[k], k
            assert np.array_equal(dev.tap(fstag.TAP_GRAY), seq[k])
        queued, rerun = dev.queue_stats()
        assert queued > 0, (queued, rerun)
    finally:
        host.close()
        dev.close()


def _jpeg(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def test_jpeg_batch_to_stag_equals_the_host_road_on_the_decoded_gray():
    """Synthetic frames as JPEG -- 4:2:0 quality 80 (compressed_image_transport's default), 4:4:4, one component, restart markers
    -- decoded on the device in one batch (JpegDecoder(max_batch=n)) and detected where they lie (detect_markers_batch_device):
    every frame == the host STag road on decode(..., to_host=True)."""
    pytest.importorskip("PIL")
    from fiducials_amd.jpeg import JpegDecoder
    w, h = 1280, 720
    words = fstag.load_library(21)
    grays = _frames(words, w, h, 5, 980, 8)
    files = [_jpeg(np.stack([grays[0]] * 3, axis=-1), quality=80, subsampling=2),
             _jpeg(tinted(grays[1], 1)[..., ::-1].copy(), quality=90, subsampling=0),
             _jpeg(grays[2], quality=85),
             _jpeg(tinted(grays[3], 3)[..., ::-1].copy(), quality=80, subsampling=2, restart_marker_blocks=7),
             _jpeg(grays[4], quality=90, restart_marker_rows=1)]
    n = len(files)
    dec = JpegDecoder(max_width=w, max_height=h, max_batch=n)
    host = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    pool = fstag.StagPool(21, 7, n_contexts=4, max_width=w, max_height=h)
    try:
        gray_host = dec.decode(files, "mono8", to_host=True)
        want = [host_result(host, g) for g in gray_host]
        assert all(x[2] >= 3 for x in want), [x[2] for x in want]
        dec.decode(files, "mono8", to_host=False)
        ptr, dw, dh, stride, fstride = dec.device_ptr()
        assert (dw, dh) == (w, h)
        M, P = pool.detect_markers_batch_device(ptr, n, w, h, stride, fstride, "mono8", K720, None, 0.18)
        for f in range(n):
            assert (M[f].tobytes(), P[f].tobytes(), len(M[f])) == want[f], f
        # one frame of the batch through the single-frame call
        m = host.detect_markers_device(ptr + 3 * fstride, w, h, stride, "mono8")
        assert m.tobytes() == want[3][0]
        assert np.array_equal(host.tap(fstag.TAP_GRAY), gray_host[3])
    finally:
        pool.close()
        host.close()
        dec.close()


def test_refusals_leave_the_context_as_it_was():
    w, h = 640, 480
    words = fstag.load_library(21)
    good, other = _frames(words, w, h, 2, 990, 6)
    t, ptr, _ = to_device(good)
    det = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    pool = fstag.StagPool(21, 7, n_contexts=2, max_width=w, max_height=h)
    L = det._L
    try:
        first = device_result(det, ptr, w, h, w, "mono8")
        assert first[2] >= 3
        gray_tap = det.tap(fstag.TAP_GRAY).tobytes()

        def refused(status, *args, **kw):
            with pytest.raises(FidError) as e:
                det.detect_markers_device(*args, **kw)
            assert e.value.status == status, (args, kw)
            # nothing of the refused call happened: the last frame's results are still what the taps and pose_last read
            assert det.markers().tobytes() == first[0] and det.tap(fstag.TAP_GRAY).tobytes() == gray_tap
            assert det.pose_last(K720, None, 0.18).tobytes() == first[1]

        for enc in ("bgra8", "rgba8", "mono16", "bayer_rggb8", "yuv422"):
            refused(_lib.FID_E_UNSUPPORTED, ptr, w, h, None, enc)
        refused(_lib.FID_E_INVALID_ARG, 0, w, h)  # null
        refused(_lib.FID_E_INVALID_ARG, ptr, w, h, w - 1)  # stride < width
        refused(_lib.FID_E_INVALID_ARG, ptr, w // 3, h, w // 3 * 3 - 1, "bgr8")  # stride < 3 width
        refused(_lib.FID_E_INVALID_ARG, ptr, w + 1, h, w + 1)  # larger than the context
        refused(_lib.FID_E_INVALID_ARG, ptr, w, h + 1)
        refused(_lib.FID_E_INVALID_ARG, ptr, 4, h)  # below the pipeline's 8 x 8
        host_buf = np.ascontiguousarray(good)
        refused(_lib.FID_E_INVALID_ARG, host_buf.ctypes.data, w, h)  # host memory
        pinned = torch.from_numpy(host_buf).pin_memory()
        refused(_lib.FID_E_INVALID_ARG, pinned.data_ptr(), w, h)  # pinned host memory: not the device's
        if torch.cuda.device_count() > 1:
            t1 = torch.from_numpy(host_buf).to("cuda:1")
            torch.cuda.synchronize(1)
            refused(_lib.FID_E_INVALID_ARG, t1.data_ptr(), w, h)  # another device's memory
        # a host call after the refused device calls on the same context
        want = host_result(det, other)
        assert want[2] >= 3
        # ... and on a fresh context
        fresh = fstag.StagDetector(21, 7, max_width=w, max_height=h)
        try:
            assert host_result(fresh, other) == want
        finally:
            fresh.close()

        # the batch entry point: the same refusals, and none of them touches the caller's counts
        cap = 16
        markers = np.zeros((3, cap), fstag.MARKER_DTYPE)
        poses = np.zeros((3, cap), fstag.POSE_DTYPE)
        counts = np.full(3, -7, np.int32)
        Kp, Dp = np.ascontiguousarray(K720).reshape(9), np.zeros(5)

        def batch(p, nframes, ww, hh, stride, fstride, enc, nctx=2, arr=None):
            return L.fid_stag_detect_markers_batch_device(arr or pool._arr, nctx, p, nframes, ww, hh, stride, fstride, enc, Kp.ctypes.data,
                                                          Dp.ctypes.data, 0.18, markers.ctypes.data, poses.ctypes.data, cap, counts.ctypes.data)

        assert batch(ptr, 1, w, h, w, w * h, 3) == _lib.FID_E_UNSUPPORTED
        assert batch(ptr, 1, w, h, w, w * h, 99) == _lib.FID_E_UNSUPPORTED
        assert batch(None, 1, w, h, w, w * h, 0) == _lib.FID_E_INVALID_ARG
        assert batch(ptr, 1, w, h, w - 1, w * h, 0) == _lib.FID_E_INVALID_ARG
        assert batch(ptr, 1, w, h, 3 * w - 1, w * h, 1) == _lib.FID_E_INVALID_ARG
        assert batch(ptr, 1, w + 1, h, w + 1, w * h, 0) == _lib.FID_E_INVALID_ARG
        assert batch(ptr, 3, w, h, w, 1 << 30, 0) == _lib.FID_E_INVALID_ARG  # frames 1 and 2 lie past the allocation
        assert batch(host_buf.ctypes.data, 1, w, h, w, w * h, 0) == _lib.FID_E_INVALID_ARG
        assert batch(ptr, 1, w, h, w, w * h, 0, nctx=0) == _lib.FID_E_INVALID_ARG
        big = fstag.StagDetector(21, 7, max_width=320, max_height=240)  # a context smaller than the frame
        try:
            arr = (C.c_void_p * 2)(pool.dets[0]._ctx.value, big._ctx.value)
            assert batch(ptr, 1, w, h, w, w * h, 0, arr=arr) == _lib.FID_E_INVALID_ARG
        finally:
            big.close()
        assert counts.tolist() == [-7, -7, -7]
        # and the pool still works
        M, P = pool.detect_markers_batch_device(ptr, 1, w, h, w, w * h, "mono8", K720, None, 0.18)
        assert M[0].tobytes() == first[0] and P[0].tobytes() == first[1]
    finally:
        pool.close()
        det.close()
    del t
