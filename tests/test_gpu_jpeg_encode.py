"""JPEG encoding on the device (fiducials_amd/csrc/fid_jpeg_enc.hip): the whole file must equal, byte for byte, the file
libjpeg-turbo wrote for the same picture -- the golden files of tests/golden/jpeg_enc_cases.npz, Pillow itself where it is
importable, and the numpy restatement (tests/jpeg_encode_restatement.py, which the CPU suite pins on both) beyond the fixture sizes.

The sizes beyond the fixtures cross the kernels' internal boundaries (the constants of fid_jpeg_enc.hip):
  SCAN_TILE  = JE_SCAN_TPB * JE_SCAN_PER = 4096 blocks a round of k_jenc_scan      -> 336 x 272 at 4:4:4 has 42 * 34 * 3 = 4284
  STUFF_TILE = JE_STUFF_TILE = 4096 entropy-coded bytes a tile of k_jenc_ffcount / k_jenc_pack -> noise at quality 100 codes to
               several hundred thousand
  CODE_TPB   = JE_TPB = 256 blocks of the scan a workgroup of k_jenc_code takes    -> 264 x 200 at 4:2:0 has MCU rows of 17 * 6 =
               102 blocks: workgroups begin and end inside MCU rows
  DCT_BLOCKS = JE_DCT_BLOCKS = 32 blocks a workgroup of k_jenc_dct                 -> every block count above that is no multiple"""
import ctypes as C
import importlib.util
import io
import os
import re

import numpy as np
import pytest

import jpeg_encode_restatement as R
from fiducials_amd import _lib
from fiducials_amd import jpeg as fj
from fiducials_amd._lib import FidError

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc_cases.npz")
MONO = 3
SCAN_TILE, STUFF_TILE, CODE_TPB = 4096, 4096, 256
HAVE_PIL = importlib.util.find_spec("PIL") is not None


def pillow(pix, q, sub):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(pix).save(b, "JPEG", quality=q, subsampling=sub)
    return b.getvalue()


def expected(pix, q, sub):
    """the file for an RGB or one-component picture: the restatement's, which must be Pillow's where Pillow is here"""
    want = R.encode(pix, q, sub)
    if HAVE_PIL:
        assert want == pillow(pix, q, sub)
    return want


def on_device(a):
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def noise_big():
    """336 x 272 RGB noise and its file at quality 100, 4:4:4 (shared: the restatement codes 4284 dense blocks)"""
    pix = np.random.default_rng(77).integers(0, 256, (272, 336, 3), dtype=np.uint8)
    st = R.Stats()
    want = R.encode(pix, 100, 0, st)
    if HAVE_PIL:
        assert want == pillow(pix, 100, 0)
    return pix, want, st


def test_every_fixture_case_from_device_and_from_host_frames(gold):
    enc = fj.JpegEncoder(max_width=64, max_height=64)
    for k, w, h, mode, q, _ in gold["cases"].tolist():
        pix = gold[f"pix_{k}"]
        want = gold[f"jpg_{k}"].tobytes()
        if HAVE_PIL:
            assert want == pillow(pix, q, 0 if mode == MONO else mode), k
        enc.set(q, 0 if mode == MONO else mode)
        name, bpp = ("mono8", 1) if mode == MONO else ("rgb8", 3)
        d = on_device(pix)
        got = enc.encode_device(d.data_ptr(), 1, w, h, w * bpp, 0, name)
        assert got == [want], (k, w, h, mode, q)
        assert enc.encode(pix, name) == [want], (k, w, h, mode, q)
    enc.close()


def test_bgr8_and_rgb8_give_the_files_of_the_swapped_pictures(gold):
    enc = fj.JpegEncoder(max_width=64, max_height=64)
    for k, w, h, mode, q, _ in gold["cases"].tolist():
        if mode == MONO or k % 3:
            continue
        pix = gold[f"pix_{k}"]
        enc.set(q, mode)
        swapped = np.ascontiguousarray(pix[..., ::-1])
        assert enc.encode(swapped, "bgr8") == [gold[f"jpg_{k}"].tobytes()]      # the same picture, stored BGR
        other = expected(swapped, q, mode)
        assert enc.encode(pix, "bgr8") == [other] == enc.encode(swapped, "rgb8")  # the picture with red and blue exchanged
    enc.close()


def test_padded_strides_mixed_batch_twice_and_two_sizes_in_turn():
    rng = np.random.default_rng(3)
    enc = fj.JpegEncoder(max_width=80, max_height=60, max_batch=4, quality=90, subsampling=1)

    def batch(w, h, q, sub, row_pad, frame_pad):
        yy, xx = np.mgrid[0:h, 0:w]
        frames = [np.random.default_rng(w * h).integers(0, 256, (h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), np.uint8),
                  np.stack([(xx * 3) % 256, (yy * 5) % 256, (xx + yy) % 256], -1).astype(np.uint8), np.full((h, w, 3), 255, np.uint8)]
        stride = w * 3 + row_pad
        fstride = stride * h + frame_pad
        buf = rng.integers(0, 256, 4 * fstride + 16, dtype=np.uint8)  # (the padding is noise: it must not be read)
        for f in range(4):
            buf[f * fstride:f * fstride + stride * h].reshape(h, stride)[:, :w * 3] = frames[f].reshape(h, w * 3)
        enc.set(q, sub)
        d = on_device(buf)
        want = [expected(fr, q, sub) for fr in frames]
        for _ in range(2):  # (twice: a word of the bit buffer that is not cleared would show in the second call)
            assert enc.encode_device(d.data_ptr(), 4, w, h, stride, fstride, "rgb8") == want, (w, h)
        return want

    big = batch(77, 53, 90, 1, 7, 13)
    small = batch(20, 9, 100, 2, 1, 0)  # a smaller size on the same context ...
    assert batch(77, 53, 90, 1, 0, 5) == big and small != big  # ... and the first again
    enc.close()


def test_more_blocks_than_a_scan_tile_more_bytes_than_a_stuffing_tile(noise_big):
    pix, want, st = noise_big
    assert st.blocks > SCAN_TILE and st.scan_bytes > 8 * STUFF_TILE and st.stuffed > 0
    enc = fj.JpegEncoder(max_width=336, max_height=272, quality=100, subsampling=0, max_file_bytes=len(want))  # (exactly its size: it fits)
    d = on_device(pix)
    assert enc.encode_device(d.data_ptr(), 1, 336, 272, 336 * 3, 0, "rgb8") == [want]
    enc.close()


def test_mcu_rows_split_between_workgroups():
    w, h = 264, 200
    assert (-(-w // 16) * 6) % CODE_TPB != 0 and CODE_TPB % (-(-w // 16) * 6) != 0
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:h, 0:w]
    pix = np.clip(np.stack([128 + 100 * np.sin(xx / 9.0), (yy * 2) % 256, 128 + 90 * np.cos(yy / 5.0 + xx / 31.0)], -1) + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)
    enc = fj.JpegEncoder(max_width=w, max_height=h, max_batch=2)
    d = on_device(np.stack([pix, pix[::-1]]))
    for q, sub in ((80, 2), (95, 1), (50, 0)):
        enc.set(q, sub)
        assert enc.encode_device(d.data_ptr(), 2, w, h, w * 3, w * h * 3, "rgb8") == [expected(pix, q, sub), expected(np.ascontiguousarray(pix[::-1]), q, sub)]
    gray = np.ascontiguousarray(pix[..., 1])
    assert enc.encode(gray, "mono8") == [expected(gray, 50, 0)]
    enc.close()


def test_full_hd_marker_frame():
    from fiducials_amd import synth
    from fiducials_amd.dictionary import get_predefined_dictionary

    gray = synth.make_frame(get_predefined_dictionary("DICT_4X4_50"), seed=11).image
    assert gray.shape == (1080, 1920)
    rgb = np.stack([gray, gray, gray], -1)
    want = pillow(rgb, 80, 2) if HAVE_PIL else R.encode(rgb, 80, 2)
    enc = fj.JpegEncoder()  # (1920 x 1080, quality 80, 4:2:0: the defaults)
    d = on_device(rgb)
    assert enc.encode_device(d.data_ptr(), 1, 1920, 1080, 1920 * 3, 0, "bgr8") == [want]
    enc.close()


def test_coefficient_tap_equals_the_restatement(gold, noise_big):
    rows = {int(r[0]): r for r in gold["cases"].tolist()}
    cases = [(gold[f"pix_{k}"], rows[k][4], rows[k][3]) for k in (14, 15, 13)]  # 17 x 23: 4:2:0 (dummy blocks right and below), one component, 4:2:2
    cases.append((noise_big[0], 100, 0))
    enc = fj.JpegEncoder(max_width=336, max_height=272, max_file_bytes=1 << 20)
    for pix, q, mode in cases:
        sub = 0 if mode == MONO else mode
        enc.set(q, sub)
        enc.encode(pix, "mono8" if pix.ndim == 2 else "rgb8")
        want = np.concatenate([c.reshape(-1) for c in R.coefficients(pix, q, sub)])
        assert np.array_equal(enc.tap(0), want), (pix.shape, q, mode)
    enc.close()


def test_a_file_that_does_not_fit_is_refused_with_its_real_size(noise_big):
    pix, want, st = noise_big
    d = on_device(pix)
    # smaller than the entropy-coded bytes alone; one byte short of the file; (the file itself fits: the test above)
    for cap in (1000, st.scan_bytes - 1, len(want) - 1):
        enc = fj.JpegEncoder(max_width=336, max_height=272, quality=100, subsampling=0, max_file_bytes=cap)
        with pytest.raises(FidError) as e:
            enc.encode_device(d.data_ptr(), 1, 336, 272, 336 * 3, 0, "rgb8")
        assert e.value.status == _lib.FID_E_CAPACITY
        assert [int(x) for x in re.findall(r"needs (\d+) bytes", str(e.value))] == [len(want)], str(e.value)
        enc.close()
    # the caller's room per file is a capacity as well, and nothing is written into it
    enc = fj.JpegEncoder(max_width=336, max_height=272, quality=100, subsampling=0, max_file_bytes=len(want))
    out = np.full(len(want), 0xA5, np.uint8)
    nb = (C.c_int64 * 1)()
    L = _lib.load()
    rc = L.fid_jpeg_encode_device(enc._ctx, C.c_void_p(d.data_ptr()), 1, 336, 272, 336 * 3, 0, _lib.ENC["rgb8"], out.ctypes.data, len(want) - 1, nb)
    assert rc == _lib.FID_E_CAPACITY and nb[0] == len(want) and (out == 0xA5).all()
    assert str(len(want)) in L.fid_jpeg_enc_last_error(enc._ctx).decode()
    rc = L.fid_jpeg_encode_device(enc._ctx, C.c_void_p(d.data_ptr()), 1, 336, 272, 336 * 3, 0, _lib.ENC["rgb8"], out.ctypes.data, len(want), nb)
    assert rc == 0 and out.tobytes() == want
    enc.close()


def test_bad_arguments_are_refused_with_a_status():
    L = _lib.load()
    INV, UNS = _lib.FID_E_INVALID_ARG, _lib.FID_E_UNSUPPORTED
    ctx = C.c_void_p()
    for args in ((0, 0, 8, 1, 0), (0, 8, 0, 1, 0), (0, 8, 8, 0, 0), (0, 16385, 8, 1, 0), (99, 8, 8, 1, 0), (0, 8, 8, 1, -1)):
        assert L.fid_jpeg_enc_create(*args, C.byref(ctx)) == INV, args
    assert L.fid_jpeg_enc_create(0, 8, 8, 1, 0, None) == INV
    enc = fj.JpegEncoder(max_width=32, max_height=16, max_batch=2)
    for q, sub in ((0, 2), (101, 2), (80, -1), (80, 3)):
        assert L.fid_jpeg_enc_set(enc._ctx, q, sub) == INV
    assert (enc.quality, enc.subsampling) == (80, 2)
    W, H = 32, 16
    d = torch.zeros(2 * W * H * 3 + 64, dtype=torch.uint8, device="cuda")
    h = np.zeros(2 * W * H * 3 + 64, np.uint8)
    out = np.zeros(2 * 4096, np.uint8)
    nb = (C.c_int64 * 2)()
    dp, hp = C.c_void_p(d.data_ptr()), C.c_void_p(h.ctypes.data)

    def dev(ctx=enc._ctx, ptr=dp, F=1, w=W, ht=H, stride=W * 3, fs=0, e=1, o=out.ctypes.data, room=4096, n=nb):
        return L.fid_jpeg_encode_device(ctx, ptr, F, w, ht, stride, fs, e, o, room, n)

    assert dev() == 0
    for e in (3, 4, 5, 9, 14, 99):  # bgra8, rgba8, a Bayer pattern, mono16, yuv422, nonsense
        assert dev(e=e) == UNS, e
    for kw in ({"ctx": None}, {"ptr": None}, {"o": None}, {"n": None}, {"F": 0}, {"F": 3}, {"w": 0}, {"ht": 0}, {"w": W + 1}, {"ht": H + 1},
               {"stride": W * 3 - 1}, {"F": 2, "fs": -1}, {"room": 0},
               {"ptr": hp},                      # host memory
               {"F": 2, "fs": 1 << 30},          # frame 1 lies past the allocation
               {"stride": 1 << 20}):             # so do the rows
        assert dev(**kw) == INV, kw
    assert dev(F=2, fs=W * H * 3) == 0 and nb[0] == nb[1] > 623
    assert L.fid_jpeg_encode(enc._ctx, hp, 1, W, H, W * 3, 0, 7, out.ctypes.data, 4096, nb) == UNS
    assert L.fid_jpeg_encode(enc._ctx, None, 1, W, H, W * 3, 0, 1, out.ctypes.data, 4096, nb) == INV
    assert L.fid_jpeg_encode(enc._ctx, hp, 1, W, H, W * 3 - 1, 0, 1, out.ctypes.data, 4096, nb) == INV
    assert L.fid_jpeg_enc_tap_bytes(enc._ctx, 5) == 0 and L.fid_jpeg_enc_tap_read(enc._ctx, 5, out.ctypes.data, 4096) == INV
    assert L.fid_jpeg_enc_tap_read(enc._ctx, 0, out.ctypes.data, 16) == _lib.FID_E_CAPACITY
    enc.close()
