"""The numpy restatement of libjpeg(-turbo)'s baseline encoder (tests/jpeg_encode_restatement.py) against the files libjpeg-turbo
wrote (tests/golden/jpeg_enc_cases.npz, tools/make_jpeg_enc_golden.py), whole file, byte for byte -- and against Pillow itself where
it is importable.  The fixture set must make the coder meet its corner cases; they are counted in the restatement."""
import importlib.util
import io
import os

import numpy as np
import pytest

import jpeg_encode_restatement as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc_cases.npz")
MONO = 3


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_restatement_equals_every_golden_file_and_the_set_meets_the_corner_cases(gold):
    st = R.Stats()
    dummy_right_420 = dummy_bottom_420 = 0
    for k, w, h, mode, q, content in gold["cases"].tolist():
        pix = gold[f"pix_{k}"]
        assert pix.shape[:2] == (h, w) and pix.ndim == (2 if mode == MONO else 3)
        one = R.Stats()
        got = R.encode(pix, q, 0 if mode == MONO else mode, one)
        assert got == gold[f"jpg_{k}"].tobytes(), (k, w, h, mode, q, content)
        for f in ("zrl", "stuffed", "dummy_right", "dummy_bottom_rows", "zero_ac_blocks", "blocks"):
            setattr(st, f, getattr(st, f) + getattr(one, f))
        st.max_category = max(st.max_category, one.max_category)
        if mode == 2:
            dummy_right_420 += one.dummy_right
            dummy_bottom_420 += one.dummy_bottom_rows
    assert st.zrl >= 1, st
    assert st.stuffed >= 1, st
    assert st.max_category >= 10, st
    assert dummy_right_420 >= 1 and dummy_bottom_420 >= 1, st
    assert st.zero_ac_blocks >= 1, st
    contents = set(gold["cases"][:, 5].tolist())
    assert {4, 5} <= contents  # flat 0 and flat 255
    assert any(q == 100 and content == 0 for _, _, _, _, q, content in gold["cases"].tolist())  # noise at quality 100


def test_restatement_equals_pillow_where_it_is_importable():
    if importlib.util.find_spec("PIL") is None:
        return  # (the golden files above are Pillow's)
    from PIL import Image

    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (17, 23), (40, 9), (31, 33), (64, 48)):
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(xx * 7 + yy) % 256, (yy * 5) % 256, (xx + yy * 2) % 256], -1).astype(np.uint8)
        for pix in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), smooth):
            for q in (1, 30, 50, 80, 95, 100):
                for sub in (0, 1, 2):
                    b = io.BytesIO()
                    Image.fromarray(pix).save(b, "JPEG", quality=q, subsampling=sub)
                    assert R.encode(pix, q, sub) == b.getvalue(), (w, h, q, sub)
                b = io.BytesIO()
                Image.fromarray(pix[..., 0]).save(b, "JPEG", quality=q)
                assert R.encode(np.ascontiguousarray(pix[..., 0]), q, 0) == b.getvalue(), (w, h, q)


def test_quantisation_tables_follow_the_quality_formula(gold):
    for k, w, h, mode, q, _ in gold["cases"].tolist():
        data = gold[f"jpg_{k}"].tobytes()
        at = data.index(b"\xff\xdb")
        table = list(data[at + 5:at + 69])
        want = R.quant_table(R.STD_LUMA, q)
        assert table == [want[R.ZIGZAG[i]] for i in range(64)], (k, q)
