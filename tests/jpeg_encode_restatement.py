"""Baseline JPEG encoding as libjpeg(-turbo) does it with its defaults, restated in numpy: the file cv::imencode(".jpg") and
PIL.Image.save(b, "JPEG", quality=q, subsampling=s) write -- sequential DCT, 8 bit, JDCT_ISLOW, the Annex K Huffman tables, one
interleaved scan for three components.  It is the CPU companion of the device encoder (fiducials_amd/csrc/fid_jpeg_enc.hip):
`encode` gives the file, `coefficients` what the device's coefficient tap must hold, `Stats` what was coded.

The rules (jccolor.c rgb_ycc_convert, jcsample.c h2v1 / h2v2_downsample, jcprepct.c, jfdctint.c, jcdctmgr.c, jccoefct.c,
jchuff.c, jcmarker.c, jcparam.c):
  colour     Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
             Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
  sampling   h2v2 (a + b + c + d + {1, 2, 1, 2, ...}) >> 2, h2v1 (a + b + {0, 1, 0, 1, ...}) >> 1; the input's right edge is
             replicated up to width_in_blocks * 8 * h_expand columns, its bottom up to a whole row group; the SAMPLED rows are then
             replicated up to height_in_blocks * 8
  transform  jpeg_fdct_islow on sample - 128, quantised by (|v| + (8 q >> 1)) / (8 q) with the sign put back
  scan       MCU by MCU; a block right of the component's width_in_blocks or below its height_in_blocks is a dummy: all zero,
             with the DC of the block in front of it in the MCU (so it codes as "difference 0, end of block")
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# ITU-T T.81 Annex K.3: (BITS, HUFFVAL) of the four tables, in the order a file carries them (DC0, AC0, DC1, AC1)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
            130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
            89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147,
            148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
            196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241,
            242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
              209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
              86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136,
              137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
              185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232,
              233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}  # Pillow's numbering -> luma sampling factors (h, v)


def quant_table(std, quality: int) -> list[int]:
    """jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((s * scale + 50) // 100, 1), 255) for s in std]


def huff_codes(spec):
    """(code, length) by symbol (jchuff.c jpeg_make_c_derived_tbl)"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(quality: int, subsampling: int, width: int, height: int, components: int) -> bytes:
    """every byte in front of the entropy-coded data (jcmarker.c write_file_header, write_frame_header, write_scan_header)"""
    def seg(marker, body):
        return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)

    hs, vs = SAMPLING[subsampling] if components == 3 else (1, 1)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t, std in enumerate([STD_LUMA, STD_CHROMA][:2 if components == 3 else 1]):
        q = quant_table(std, quality)
        out += seg(0xDB, [t] + [q[ZIGZAG[k]] for k in range(64)])
    sof = [8, height >> 8, height & 255, width >> 8, width & 255, components]
    for c in range(components):
        sof += [c + 1, (hs << 4 | vs) if c == 0 else 0x11, 0 if c == 0 else 1]
    out += seg(0xC0, sof)
    for tc_th, spec in [(0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)][:4 if components == 3 else 2]:
        out += seg(0xC4, [tc_th] + spec[0] + spec[1])
    sos = [components]
    for c in range(components):
        sos += [c + 1, 0x00 if c == 0 else 0x11]
    return out + seg(0xDA, sos + [0, 63, 0])


def _fdct_pass(d, first):
    """one pass of jpeg_fdct_islow along the last axis (13-bit constants, PASS1_BITS = 2)"""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15

    def ds(x, s):
        return (x + (1 << (s - 1))) >> s

    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else ds(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else ds(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = ds(z1 + t13 * 6270, n)
    o[6] = ds(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
    return np.stack(o, -1)


def _blocks(plane, q):
    """quantised coefficients [bh][bw][64], natural order, of a plane whose sides are multiples of 8"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.astype(np.int64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    b = _fdct_pass(b, True)                                      # rows
    b = _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)  # columns
    q8 = np.asarray(q, np.int64).reshape(8, 8) * 8
    return (np.sign(b) * ((np.abs(b) + (q8 >> 1)) // q8)).reshape(bh, bw, 64).astype(np.int16)


def _edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def sample_planes(img: np.ndarray, subsampling: int):
    """-> per component the sample plane the transform reads (real blocks only): colour conversion, edge expansion, downsampling"""
    H, W = img.shape[:2]
    if img.ndim == 2:
        return [_edge(img, -(-H // 8) * 8, -(-W // 8) * 8)]
    hs, vs = SAMPLING[subsampling]
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    out = [_edge(y, -(-H // 8) * 8, -(-W // 8) * 8)]
    cw, ch = -(-W // hs), -(-H // vs)
    cbw, cbh = -(-cw // 8), -(-ch // 8)
    for c in (cb, cr):
        e = _edge(c, ch * vs, cbw * 8 * hs)  # the input: right edge to the sampled width, bottom to a whole row group
        if (hs, vs) == (2, 2):
            bias = np.tile([1, 2], cbw * 4)
            e = (e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2] + bias) >> 2
        elif (hs, vs) == (2, 1):
            bias = np.tile([0, 1], cbw * 4)
            e = (e[:, 0::2] + e[:, 1::2] + bias) >> 1
        out.append(_edge(e, cbh * 8, cbw * 8))  # the sampled rows: bottom to whole blocks
    return out


def geometry(width: int, height: int, components: int, subsampling: int):
    """-> (hs, vs, mcux, mcuy, [(real blocks w, h, scan blocks w, h) per component]); one component: a scan of its own blocks, no
    dummies (jccoefct.c: MCU = one block); three: MCU-padded"""
    if components == 1:
        bw, bh = -(-width // 8), -(-height // 8)
        return 1, 1, bw, bh, [(bw, bh, bw, bh)]
    hs, vs = SAMPLING[subsampling]
    mcux, mcuy = -(-width // (8 * hs)), -(-height // (8 * vs))
    comps = [(-(-width // 8), -(-height // 8), mcux * hs, mcuy * vs)]
    cw, ch = -(-width // hs), -(-height // vs)
    comps += [(-(-cw // 8), -(-ch // 8), mcux, mcuy)] * 2
    return hs, vs, mcux, mcuy, comps


def coefficients(img: np.ndarray, quality: int, subsampling: int):
    """-> per component int16 [scan blocks h][scan blocks w][64], natural order, DC not yet predicted: the layout of
    FID_JPEG_TAP_COEFS and of the encoder's tap.  Dummy blocks are all zero but for the DC of the block in front of them in the MCU."""
    H, W = img.shape[:2]
    nc = 1 if img.ndim == 2 else 3
    hs, vs, mcux, mcuy, comps = geometry(W, H, nc, subsampling)
    planes = sample_planes(img, subsampling)
    qt = [quant_table(STD_LUMA, quality)] + [quant_table(STD_CHROMA, quality)] * 2
    out = []
    for c in range(nc):
        rw, rh, sw, sh = comps[c]
        real = _blocks(planes[c], qt[c])
        assert real.shape[:2] == (rh, rw)
        full = np.zeros((sh, sw, 64), np.int16)
        full[:rh, :rw] = real
        out.append(full)
    if nc == 3:  # the luma dummies take the DC of the block in front of them in MCU order (row by row inside the MCU)
        rw, rh, sw, sh = comps[0]
        y = out[0]
        for my in range(mcuy):
            for mx in range(mcux):
                prev = None
                for i in range(hs * vs):
                    by, bx = my * vs + i // hs, mx * hs + i % hs
                    if by >= rh or bx >= rw:
                        y[by, bx, 0] = prev
                    prev = y[by, bx, 0]
    return out


@dataclass
class Stats:
    zrl: int = 0               # ZRL symbols (0xF0) coded
    stuffed: int = 0           # 0x00 bytes stuffed behind a 0xFF
    max_category: int = 0      # largest size category of a coefficient (or DC difference)
    dummy_right: int = 0       # dummy blocks right of a component's width_in_blocks (in rows that have real blocks)
    dummy_bottom_rows: int = 0  # block rows of dummy blocks below a component's height_in_blocks
    zero_ac_blocks: int = 0    # real blocks whose 63 AC coefficients are all zero
    blocks: int = 0
    scan_bytes: int = 0        # entropy-coded bytes before stuffing


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.raw = 0
        self.stuffed = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            self.raw += 1
            if byte == 255:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)  # (pad with 1-bits)


_TABLES = None


def _tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = [huff_codes(s) for s in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)]
    return _TABLES


def encode(img: np.ndarray, quality: int = 80, subsampling: int = 2, stats: Stats | None = None) -> bytes:
    """img: [H][W] uint8 (one component) or [H][W][3] RGB.  -> the whole file."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and 1 <= quality <= 100
    H, W = img.shape[:2]
    nc = 1 if img.ndim == 2 else 3
    st = stats if stats is not None else Stats()
    hs, vs, mcux, mcuy, comps = geometry(W, H, nc, subsampling)
    coefs = coefficients(img, quality, subsampling)
    zz = np.asarray(ZIGZAG)
    dc0, ac0, dc1, ac1 = _tables()
    w = _Bits()
    pred = [0, 0, 0]
    for c in range(nc):
        rw, rh, sw, sh = comps[c]
        st.dummy_bottom_rows += (sh - rh) * 1
        st.dummy_right += (sw - rw) * rh

    def block(c, by, bx):
        v = coefs[c][by, bx]
        rw, rh = comps[c][:2]
        dct, act = (dc0, ac0) if c == 0 else (dc1, ac1)
        st.blocks += 1
        diff = int(v[0]) - pred[c]
        pred[c] = int(v[0])
        nb = abs(diff).bit_length()
        st.max_category = max(st.max_category, nb)
        w.put(*dct[nb])
        if nb:
            w.put((diff if diff >= 0 else diff - 1) & ((1 << nb) - 1), nb)
        z = v[zz]
        nz = np.flatnonzero(z[1:]) + 1
        if nz.size == 0 and by < rh and bx < rw:
            st.zero_ac_blocks += 1
        last = 0
        for k in nz:
            run = int(k) - last - 1
            while run > 15:
                w.put(*act[0xF0])
                st.zrl += 1
                run -= 16
            a = int(z[k])
            nb = abs(a).bit_length()
            st.max_category = max(st.max_category, nb)
            w.put(*act[run << 4 | nb])
            w.put((a if a >= 0 else a - 1) & ((1 << nb) - 1), nb)
            last = int(k)
        if last != 63:
            w.put(*act[0])

    for my in range(mcuy):
        for mx in range(mcux):
            if nc == 1:
                block(0, my, mx)
                continue
            for i in range(hs * vs):
                block(0, my * vs + i // hs, mx * hs + i % hs)
            block(1, my, mx)
            block(2, my, mx)
    w.finish()
    st.stuffed += w.stuffed
    st.scan_bytes += w.raw
    return header(quality, subsampling, W, H, nc) + bytes(w.out) + b"\xff\xd9"
