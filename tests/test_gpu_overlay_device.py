"""The /fiducial_images overlay on frames in device memory (k_to_bgr, k_draw_markers): fid_to_bgr_device,
fid_draw_detected_markers_device and fid_jpeg_marker_image must give, byte for byte and frame by frame, what the host calls
fid_to_bgr / fid_draw_detected_markers give -- every octant and slope, clipping, corners far outside the int range, the write
order of the two colours -- and refuse what the host calls refuse.  Padding around the frames must stay untouched."""
import ctypes as C
import io

import numpy as np
import pytest

from fiducials_amd import _lib, overlay
from fiducials_amd._lib import FidMarker

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0xA5
BPP = {"mono8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}


def L():
    return _lib.load()


def markers_array(quads_per_frame, cap):
    mk = (FidMarker * max(len(quads_per_frame) * cap, 1))()
    for f, q in enumerate(quads_per_frame):
        q = np.asarray(q, np.float32).reshape(-1, 8)
        for i in range(len(q)):
            mk[f * cap + i].id = i
            for j in range(8):
                mk[f * cap + i].corners[j] = float(q[i, j])
    return mk


def host_draw(img, quads, flags):
    return overlay.draw_detected_markers(img.copy(), np.asarray(quads, np.float32).reshape(-1, 4, 2), None, flags)


def check_draw(W, H, quads_per_frame, flags, seed=0, row_pad=7, frame_pad=13):
    """quads_per_frame: one (n, 4, 2) array per frame; the frames lie row_pad bytes of padding per row and frame_pad bytes
    between frames apart in one device buffer.  Device result == host result frame by frame, padding untouched."""
    rng = np.random.default_rng(seed)
    F = len(quads_per_frame)
    stride = W * 3 + row_pad
    fstride = stride * H + frame_pad
    base = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    buf = np.full(F * fstride + 64, FILL, np.uint8)
    for f in range(F):
        buf[f * fstride:f * fstride + stride * H].reshape(H, stride)[:, :W * 3] = base[f].reshape(H, W * 3)
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    cap = max(max(len(np.asarray(q).reshape(-1, 8)) for q in quads_per_frame), 1)
    cnt = (C.c_int32 * F)(*[len(np.asarray(q).reshape(-1, 8)) for q in quads_per_frame])
    rc = L().fid_draw_detected_markers_device(C.c_void_p(d.data_ptr()), F, W, H, stride, fstride, markers_array(quads_per_frame, cap), cap, cnt, flags)
    assert rc == 0, rc
    got = d.cpu().numpy()
    want = buf.copy()
    for f in range(F):
        want[f * fstride:f * fstride + stride * H].reshape(H, stride)[:, :W * 3] = host_draw(base[f], quads_per_frame[f], flags).reshape(H, W * 3)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:5]}"
    return [want[f * fstride:f * fstride + stride * H].reshape(H, stride)[:, :W * 3].reshape(H, W, 3) for f in range(F)], base


# ---- fid_to_bgr_device

@pytest.mark.parametrize("enc", list(BPP))
def test_to_bgr_device_equals_host(enc):
    bpp = BPP[enc]
    rng = np.random.default_rng(bpp)
    for W, H, F, spad, dpad in ((53, 37, 3, 5, 7), (64, 24, 2, 16 * bpp, 16), (1, 1, 1, 0, 0), (50, 1, 4, 3, 0)):
        sstride, dstride = W * bpp + spad, W * 3 + dpad
        sfstride, dfstride = sstride * H + 11, dstride * H + 32
        src = rng.integers(0, 256, F * sfstride + 16, dtype=np.uint8)
        dst = np.full(F * dfstride + 16, FILL, np.uint8)
        ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        torch.cuda.synchronize()
        rc = L().fid_to_bgr_device(C.c_void_p(ds.data_ptr()), F, W, H, sstride, sfstride, _lib.ENC[enc], C.c_void_p(dd.data_ptr()), dstride, dfstride)
        assert rc == 0, (enc, W, H, rc)
        got = dd.cpu().numpy()
        want = dst.copy()
        for f in range(F):
            fr = np.lib.stride_tricks.as_strided(src[f * sfstride:], (H, W * bpp), (sstride, 1))
            fr = fr.reshape(H, W) if bpp == 1 else fr.reshape(H, W, bpp)
            want[f * dfstride:f * dfstride + dstride * H].reshape(H, dstride)[:, :W * 3] = overlay.to_bgr(fr, enc).reshape(H, W * 3)
        assert np.array_equal(got, want), (enc, W, H, int((got != want).sum()))


def test_to_bgr_device_1080p_batch_wide_path():
    """a batch of 1080p BGRA frames in a tight layout: every 16-pixel chunk takes the 16-byte loads and stores"""
    rng = np.random.default_rng(4)
    src = torch.from_numpy(rng.integers(0, 256, (3, 1080, 1920, 4), dtype=np.uint8)).cuda()
    out = overlay.to_bgr_device(src, "rgba8")
    s = src.cpu().numpy()
    o = out.cpu().numpy()
    for f in range(3):
        assert np.array_equal(o[f], overlay.to_bgr(s[f], "rgba8"))


# ---- fid_draw_detected_markers_device

def random_quads(rng, W, H, n=60):
    quads = []
    for _ in range(n):
        c = rng.uniform([40, 40], [W - 40, H - 40])
        a = rng.uniform(0, 2 * np.pi)
        r = rng.uniform(5, 120)
        ang = a + np.array([0, 0.5, 1.0, 1.5]) * np.pi + rng.uniform(-0.2, 0.2, 4)
        quads.append(np.stack([c[0] + r * np.cos(ang), c[1] + r * np.sin(ang)], 1))
    q = np.array(quads, dtype=np.float32)
    q[0] = [[10.5, 10.5], [11.5, 10.5], [11.5, 11.5], [10.5, 11.5]]  # halves round to even
    return q


@pytest.mark.parametrize("flags", [0, 1])
def test_draw_device_random_quads(flags):
    rng = np.random.default_rng(8)
    frames = [random_quads(rng, 640, 480), random_quads(rng, 640, 480, 20)]
    imgs, base = check_draw(640, 480, frames, flags)
    assert (imgs[0] != base[0]).any()


@pytest.mark.parametrize("flags", [0, 1])
def test_draw_device_every_octant_and_slope(flags):
    """lines from one centre to every pixel of a square ring of radius 300, each drawn both ways (C -> P and P -> C)"""
    cx = cy = 310
    r = 300
    ring = [(x, cy - r) for x in range(cx - r, cx + r)] + [(cx + r, y) for y in range(cy - r, cy + r)] + \
           [(x, cy + r) for x in range(cx + r, cx - r, -1)] + [(cx - r, y) for y in range(cy + r, cy - r, -1)]
    q = np.array([[[cx, cy], [px, py], [cx, cy], [px, py]] for px, py in ring], np.float32)
    assert len(q) == 2400
    check_draw(621, 621, [q[:1200], q[1200:]], flags)
    # sub-pixel end points (the rounding of Point2f -> Point) on a few hundred of them
    rng = np.random.default_rng(3)
    q2 = q[::6] + rng.uniform(-0.5, 0.5, q[::6].shape).astype(np.float32)
    check_draw(621, 621, [q2], flags)


@pytest.mark.parametrize("flags", [0, 1])
def test_draw_device_long_lines(flags):
    rng = np.random.default_rng(11)
    W, H = 4096, 300
    q = []
    for _ in range(12):
        x0, x1 = rng.uniform(0, 60), rng.uniform(4030, 4095)
        y = rng.uniform(0, H - 1, 4)
        q.append([[x0, y[0]], [x1, y[1]], [x1 - rng.uniform(0, 30), y[2]], [x0 + rng.uniform(0, 30), y[3]]])
    check_draw(W, H, [np.array(q, np.float32)], flags, row_pad=0, frame_pad=0)


@pytest.mark.parametrize("flags", [0, 1])
def test_draw_device_outside_the_frame_and_out_of_range(flags):
    rng = np.random.default_rng(5)
    W, H = 320, 240
    partly = rng.uniform([-W, -H], [2 * W, 2 * H], (80, 4, 2)).astype(np.float32)
    wholly = (rng.uniform([W + 10, 0], [3 * W, H], (20, 4, 2))).astype(np.float32)
    wholly2 = (rng.uniform([-3 * W, -3 * H], [-10, -10], (20, 4, 2))).astype(np.float32)
    bad = [np.inf, -np.inf, np.nan, 1e9, -1e9, 1e18, -1e18, 3e9, -3e9, 2147483648.0, -2147483904.0, 2147483520.0]
    odd = rng.uniform([0, 0], [W, H], (120, 4, 2)).astype(np.float32)
    for k in range(len(odd)):
        for _ in range(int(rng.integers(1, 4))):
            odd[k, rng.integers(0, 4), rng.integers(0, 2)] = bad[int(rng.integers(0, len(bad)))]
    same = np.repeat(rng.uniform([0, 0], [W, H], (10, 1, 2)).astype(np.float32), 4, axis=1)  # all four corners equal
    big = np.array([[[1e9, 1e9], [-1e9, 1e9], [-1e9, -1e9], [1e9, -1e9]], [[-1e9, 100], [1e9, 120], [1e9, 130], [-1e9, 110]]], np.float32)
    check_draw(W, H, [partly, wholly, wholly2, odd, same, big], flags)


@pytest.mark.parametrize("flags", [0, 1])
def test_draw_device_tiny_images(flags):
    rng = np.random.default_rng(9)
    check_draw(1, 1, [rng.uniform(-2, 3, (30, 4, 2)).astype(np.float32), np.zeros((1, 4, 2), np.float32)], flags)
    check_draw(50, 1, [rng.uniform([-10, -2], [60, 3], (40, 4, 2)).astype(np.float32)], flags)
    check_draw(1, 40, [rng.uniform([-2, -10], [3, 50], (40, 4, 2)).astype(np.float32)], flags)


def test_draw_device_batch_mixes_empty_and_full_frames():
    rng = np.random.default_rng(12)
    full = [random_quads(rng, 200, 150, 30) for _ in range(3)]
    empty = np.zeros((0, 4, 2), np.float32)
    for flags in (0, 1):
        imgs, base = check_draw(200, 150, [empty, full[0], empty, full[1], full[2], empty], flags)
        assert np.array_equal(imgs[0], base[0]) and np.array_equal(imgs[5], base[5]) and not np.array_equal(imgs[1], base[1])


def test_draw_device_write_order_of_the_two_colours():
    """marker i + 1's green side crosses marker i's red first-corner square (green must win there), and marker i's green side is
    crossed by marker i + 1's red square (red must win): the host's order, which a device without it would not keep"""
    m0 = [[100, 100], [160, 100], [160, 160], [100, 160]]  # its red square spans x, y in 97 .. 103
    m1 = [[60, 101], [140, 101], [140, 130], [60, 130]]    # its top side runs through m0's square along y = 101
    m2 = [[60, 200], [140, 200], [140, 240], [60, 240]]    # its top side y = 200 ...
    m3 = [[100, 199], [120, 180], [130, 190], [110, 220]]  # ... is crossed by m3's red square (97 .. 103, 196 .. 202)
    q = np.array([m0, m1, m2, m3], np.float32)
    imgs, _ = check_draw(200, 260, [q], 1)
    img = imgs[0]
    assert (img[101, 97] == (0, 255, 0)).all() and (img[97, 100] == (0, 0, 255)).all()
    assert (img[200, 97] == (0, 0, 255)).all() and (img[200, 90] == (0, 255, 0)).all()


def test_draw_device_refusals_match_the_host():
    W, H = 32, 16
    d = torch.zeros(W * 3 * H + 64, dtype=torch.uint8, device="cuda")
    h = np.zeros(W * 3 * H + 64, np.uint8)
    mk = markers_array([np.zeros((1, 4, 2), np.float32)], 1)
    one = (C.c_int32 * 1)(1)
    dp, hp = C.c_void_p(d.data_ptr()), h.ctypes.data_as(C.c_void_p)
    INV = _lib.FID_E_INVALID_ARG

    def dev(ptr=dp, F=1, w=W, ht=H, stride=W * 3, fs=0, m=mk, cap=1, n=one, flags=0):
        return L().fid_draw_detected_markers_device(ptr, F, w, ht, stride, fs, m, cap, n, flags)

    def host(w=W, ht=H, stride=W * 3, m=mk, n=1, flags=0):
        return L().fid_draw_detected_markers(hp, w, ht, stride, m, n, flags)

    assert dev() == host() == 0
    for kw in ({"flags": 2}, {"stride": W * 3 - 1}, {"w": 0}, {"ht": 0}):
        assert dev(**kw) == host(**kw) == INV, kw
    assert dev(n=(C.c_int32 * 1)(-1)) == host(n=-1) == INV
    assert dev(n=(C.c_int32 * 1)(2)) == INV                    # more markers than cap_per_frame
    assert dev(cap=4097, n=(C.c_int32 * 1)(0)) == INV          # cap_per_frame above the marker limit
    assert dev(m=None) == host(m=None) == INV
    assert dev(ptr=hp) == INV                                  # host memory
    assert dev(F=2, fs=1 << 30, n=(C.c_int32 * 2)(0, 1)) == INV  # frame 1 lies past the allocation
    assert dev(F=2, fs=W * 3 * H - 1, n=(C.c_int32 * 2)(0, 0)) == INV  # frames that overlap
    # fid_to_bgr_device: the host call's refusals, and memory that is not the device's
    d2 = torch.zeros(W * 3 * H + 64, dtype=torch.uint8, device="cuda")
    dq = C.c_void_p(d2.data_ptr())
    assert L().fid_to_bgr_device(dp, 1, W, H, W, 0, 0, dq, W * 3, 0) == 0
    for enc in (9, 5, 14, 99):  # mono16, a Bayer pattern, yuv422, nonsense
        assert L().fid_to_bgr_device(dp, 1, W, H, W * 8, 0, enc, dq, W * 3, 0) == INV
        assert L().fid_to_bgr(hp, W, H, W * 8, enc, hp, C.c_int64(h.nbytes)) == INV
    assert L().fid_to_bgr_device(dp, 1, W, H, W * 3 - 1, 0, 1, dq, W * 3, 0) == INV == L().fid_to_bgr(hp, W, H, W * 3 - 1, 1, hp, C.c_int64(h.nbytes))
    assert L().fid_to_bgr_device(dp, 1, W, H, W, 0, 0, dq, W * 3 - 1, 0) == INV
    assert L().fid_to_bgr_device(hp, 1, W, H, W, 0, 0, dq, W * 3, 0) == INV
    assert L().fid_to_bgr_device(dp, 2, W, H, W, 1 << 30, 0, dq, W * 3, W * 3 * H) == INV  # source past its allocation
    assert L().fid_to_bgr_device(dp, 2, W, H, W, 0, 0, dq, W * 3, 1 << 30) == INV           # destination past its allocation
    assert L().fid_to_bgr_device(dp, 1, W, H, W, 0, 0, dp, W * 3, 0) == INV           # in place


# ---- the torch wrappers

def test_torch_wrappers_match_the_host_overlay_on_strided_views():
    rng = np.random.default_rng(21)
    big = torch.from_numpy(rng.integers(0, 256, (3, 40, 64, 4), dtype=np.uint8)).cuda()
    src = big[:, :, 5:55]                                   # strided rows: 64 * 4 bytes apart, 50 pixels each
    out_big = torch.full((3, 44, 70, 3), FILL, dtype=torch.uint8, device="cuda")
    out = out_big[:, 2:42, 3:53]
    assert overlay.to_bgr_device(src, "rgba8", out=out) is out
    s = src.cpu().numpy()
    quads = [random_quads(rng, 500, 400, 5) * 0.1, np.zeros((0, 4, 2), np.float32), random_quads(rng, 500, 400, 9) * 0.1]
    assert overlay.draw_detected_markers_device(out, quads, [np.arange(5), np.arange(0), np.arange(9)], overlay.FIRST_CORNER_LINE8) is out
    ob = out_big.cpu().numpy()
    for f in range(3):
        want = overlay.draw_detected_markers(overlay.to_bgr(s[f], "rgba8"), quads[f], None, overlay.FIRST_CORNER_LINE8)
        assert np.array_equal(ob[f, 2:42, 3:53], want)
    ob[:, 2:42, 3:53] = FILL
    assert (ob == FILL).all()  # nothing outside the view was written
    # one frame [H, W, C], mono8
    g = torch.from_numpy(rng.integers(0, 256, (30, 20, 1), dtype=np.uint8)).cuda()
    one = overlay.to_bgr_device(g)
    overlay.draw_detected_markers_device(one, quads[0] * 0.5)
    want = overlay.draw_detected_markers(overlay.to_bgr(g.cpu().numpy()[..., 0]), quads[0] * 0.5)
    assert np.array_equal(one.cpu().numpy(), want)
    with pytest.raises(ValueError):
        overlay.draw_detected_markers_device(big, [quads[0]] * 3)  # four channels


# ---- fid_jpeg_marker_image

def test_jpeg_marker_image_equals_decode_then_host_draw():
    from PIL import Image

    from fiducials_amd import jpeg as fj

    rng = np.random.default_rng(30)
    rgb = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=85)
    data = b.getvalue()
    dec = fj.JpegDecoder(max_width=160, max_height=120)
    q = random_quads(rng, 160, 120, 8) * 0.3
    mk = markers_array([q], len(q))
    out = np.zeros((120, 160, 3), np.uint8)
    for enc in ("bgr8", "mono8"):
        img = dec.decode(data, enc)
        base = overlay.to_bgr(img.reshape(120, 160, -1)[..., 0] if enc == "mono8" else img.reshape(120, 160, 3))
        for flags, n in ((0, len(q)), (1, len(q)), (0, 0)):
            rc = L().fid_jpeg_marker_image(dec._ctx, 0, _lib.ENC[enc], mk, n, flags, out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes))
            assert rc == 0, rc
            assert np.array_equal(out, host_draw(base, q[:n], flags) if n else base), (enc, flags, n)
        other = _lib.ENC["mono8" if enc == "bgr8" else "bgr8"]
        assert L().fid_jpeg_marker_image(dec._ctx, 0, other, mk, 1, 0, out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes)) == _lib.FID_E_INVALID_ARG
    ptr = out.ctypes.data_as(C.c_void_p)
    assert L().fid_jpeg_marker_image(dec._ctx, 0, _lib.ENC["mono8"], mk, 1, 0, ptr, C.c_int64(out.nbytes - 1)) == _lib.FID_E_CAPACITY
    assert L().fid_jpeg_marker_image(dec._ctx, 1, _lib.ENC["mono8"], mk, 1, 0, ptr, C.c_int64(out.nbytes)) == _lib.FID_E_INVALID_ARG
    assert L().fid_jpeg_marker_image(dec._ctx, 0, _lib.ENC["mono8"], mk, 4097, 0, ptr, C.c_int64(out.nbytes)) == _lib.FID_E_INVALID_ARG
    assert L().fid_jpeg_marker_image(dec._ctx, 0, _lib.ENC["mono8"], mk, 1, 2, ptr, C.c_int64(out.nbytes)) == _lib.FID_E_INVALID_ARG
    dec.close()
