#!/usr/bin/env python3
"""JPEG fixtures for the device encoder: tests/golden/jpeg_enc_cases.npz.  Every case is a small picture (its pixels are stored:
[H][W] for one component, [H][W][3] RGB for three) and the file libjpeg-turbo (Pillow) writes for it at the case's quality and
chroma sampling -- what cv::imencode(".jpg") writes.  The set is chosen so that the coder meets ZRL symbols, stuffed 0xFF bytes,
coefficients of the largest size categories, dummy blocks on the right edge and in the bottom MCU row, and blocks without AC
coefficients (tests/test_jpeg_encode_restatement.py counts them).  Needs Pillow."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (9, 40), (33, 31), (48, 50), (15, 16), (16, 15), (25, 7)]
NOISE, GRADIENT, SQUARE, BLOCKS, FLAT0, FLAT255 = range(6)
MONO = 3  # mode: 0 / 1 / 2 = three components at Pillow's subsampling 4:4:4 / 4:2:2 / 4:2:0, 3 = one component


def picture(w, h, content, seed, mono):
    rng = np.random.default_rng(seed)
    ch = () if mono else (3,)
    if content == NOISE:
        a = rng.integers(0, 256, (h, w) + ch)
    elif content == GRADIENT:
        yy, xx = np.mgrid[0:h, 0:w]
        a = (xx * 5 + yy * 3) % 256 if mono else np.stack([(xx * 5 + yy * 3) % 256, (xx * 2 + 40) % 256, (yy * 7 + xx) % 256], -1)
    elif content == SQUARE:
        a = rng.normal(60, 6, (h, w) + ch)
        a[h // 4:h - h // 4, w // 4:w - w // 4] = 200 + rng.normal(0, 6, a[h // 4:h - h // 4, w // 4:w - w // 4].shape)
    elif content == BLOCKS:  # whole 8 x 8 blocks of 0 or 255: the largest DC differences
        by, bx = -(-h // 8), -(-w // 8)
        a = np.kron(rng.integers(0, 2, (by, bx)) * 255, np.ones((8, 8), np.int64))[:h, :w]
        a = a if mono else np.stack([a, a, a], -1)
    else:
        a = np.full((h, w) + ch, 0 if content == FLAT0 else 255)
    return np.clip(a, 0, 255).astype(np.uint8)


def case_list():
    cases = []
    for i, (w, h) in enumerate(SIZES):
        for mode in range(4):
            cases.append((w, h, mode, [30, 80, 95, 100][(i + mode) % 4], [NOISE, GRADIENT, SQUARE][(i + 2 * mode) % 3]))
    for mode in range(4):  # the qualities the header test covers, on every layout
        for q in (1, 50, 80, 100):
            cases.append((17, 23, mode, q, SQUARE))
    for mode in range(4):
        cases.append((33, 31, mode, 100, NOISE))
        cases.append((33, 31, mode, 100, BLOCKS))
    cases += [(48, 50, 2, 100, NOISE), (17, 23, 2, 80, FLAT0), (17, 23, 2, 80, FLAT255), (16, 16, 0, 95, FLAT0), (25, 7, MONO, 100, FLAT255),
              (48, 50, 1, 30, GRADIENT), (9, 40, 2, 100, BLOCKS)]
    return cases


def main():
    out = {}
    rows = []
    for k, (w, h, mode, q, content) in enumerate(case_list()):
        a = picture(w, h, content, 1000 + k, mode == MONO)
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", quality=q, subsampling=0 if mode == MONO else mode)
        out[f"pix_{k}"] = a
        out[f"jpg_{k}"] = np.frombuffer(b.getvalue(), np.uint8)
        rows.append((k, w, h, mode, q, content))
    out["cases"] = np.array(rows, np.int32)
    out["made_with"] = np.array([f"Pillow libjpeg {features.version('jpg')} turbo={features.check_feature('libjpeg_turbo')}"])
    path = os.path.join(ROOT, "tests", "golden", "jpeg_enc_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(rows), "cases")


if __name__ == "__main__":
    sys.exit(main())
