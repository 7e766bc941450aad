"""The reference-built STag oracle (oracle/_ref): loads, and its pieces behave as the reference code reads."""
import os

import numpy as np
import pytest

from oracle import stag_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_constants_are_the_reference_ones():
    _need_ref()
    assert stag_ref.constants() == dict(EDGE_VERTICAL=1, EDGE_HORIZONTAL=2, ANCHOR_PIXEL=254)


def test_smooth5_is_the_fixed_binomial_kernel():
    _need_ref()
    img = np.zeros((9, 9), np.uint8)
    img[4, 4] = 255
    s = stag_ref.smooth5(img)
    k = np.array([1, 4, 6, 4, 1])
    assert np.array_equal(s[2:7, 2:7], (np.outer(k, k) * 255 + 128) >> 8)
    assert stag_ref.smooth5(np.full((5, 7), 93, np.uint8)).tolist() == [[93] * 7] * 5  # reflect-101 keeps a constant


def test_vertical_step_edge_gives_vertical_anchors_sorted_by_gradient():
    _need_ref()
    img = np.zeros((12, 16), np.uint8)
    img[:, 8:] = 200
    grad, dirs = stag_ref.gradient(img, 16)
    assert (grad[0, :] == 15).all() and (grad[:, 0] == 15).all()  # border = GRADIENT_THRESH - 1
    assert grad[5, 7] == 600 and grad[5, 8] == 600 and dirs[5, 7] == 1
    edge, order = stag_ref.anchors(grad, dirs, 16, 0, 1)
    ys, xs = np.nonzero(edge)
    assert set(xs.tolist()) == {7, 8} and ys.min() == 2 and ys.max() == 9
    g = grad.reshape(-1)[order]
    assert (np.diff(g) >= 0).all()
    # equal gradients: descending offsets (the --C[grad] placement of SortAnchorsByGradValue)
    assert (np.diff(order) < 0).all()


def _need_ref():
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")


def test_piecewise_calls_equal_the_reference_pipeline_end_to_end():
    """The stage-by-stage entry points the GPU parity tests use (gradient, anchors, routing, validation, line fitting) give,
    chained, exactly what the reference's DetectLinesByEDPF returns in one go: the wrappers add nothing of their own."""
    _need_ref()
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:240, 0:320]
    img = (150 + 30 * np.sin(xx / 40.0) + rng.normal(0, 2, (240, 320))).astype(np.float64)
    img[60:180, 80:220] = 30
    img[(yy - 120) ** 2 + (xx - 150) ** 2 < 45 ** 2] = 220
    img = np.clip(img, 0, 255).astype(np.uint8)
    lines, segs, pix = stag_ref.detect_lines(img)
    sm = stag_ref.smooth5(img)
    g, d = stag_ref.gradient(sm, 16)
    e, order = stag_ref.anchors(g, d, 16, 0, 1)
    _, rp, rs = stag_ref._route_raw(g, d, e)
    _, vs = stag_ref.validate(stag_ref.smooth3(img), rp, rs)
    l2, mll = stag_ref.fit_lines(img, rp, vs, validate=True)
    assert mll >= 9 and len(lines) > 4
    assert np.array_equal(vs, segs) and np.array_equal(l2, lines)
    for a, n in segs:
        assert np.array_equal(rp[a:a + n], pix[a:a + n])


def test_marker_libraries_are_the_published_tables():
    """fiducials_amd/data/stag_HD*.bin (tools/make_stag_libraries.py): sizes of Decoder.cpp:17-37, 48-bit words, four
    blocks per library, no word twice, block k = block 0 turned by k quarter turns of the code ring."""
    from fiducials_amd.stag import load_library
    sizes = {11: 22309, 13: 2884, 15: 766, 17: 157, 19: 38, 21: 12, 23: 6}
    for hd, n in sizes.items():
        w = load_library(hd)
        assert w.dtype == np.uint64 and len(w) == 4 * n and int(w.max()) < (1 << 48)
        assert len(np.unique(w)) == len(w)
        # the four blocks are the four quarter turns of the code ring (12 of the 48 code points per quadrant, Stag.cpp:139-173)
        mask = np.uint64((1 << 48) - 1)
        for k in range(1, 4):
            sh = (36 * k) % 48
            rot = ((w[:n] << np.uint64(sh)) | (w[:n] >> np.uint64(48 - sh))) & mask
            assert np.array_equal(w[k * n:(k + 1) * n], rot), (hd, k)


@pytest.mark.parametrize("hd,ec", [(21, 7), (17, 5)])
def test_rendered_codewords_come_back_from_the_reference_detector(hd, ec):
    """Known-answer test for the checker itself: markers rendered from library codewords (fiducials_amd.synth) go through the
    reference's Stag::detectMarkers (oracle/_ref: the reference's sources + the restated OpenCV calls) and the ids read are
    ids that were drawn, at the drawn places."""
    _need_ref()
    from fiducials_amd import synth
    from fiducials_amd.stag import load_library
    words = load_library(hd)
    fr = synth.make_stag_frame(words, 5, 1280, 720, 8)
    m = stag_ref.detect_markers(fr.image, hd, ec, refine=True)
    assert len(m) >= 4
    for row in m:
        js = np.flatnonzero(fr.ids == int(row[0]))
        assert len(js) > 0, "an id that was never drawn"
        assert min(np.abs(row[1:9].reshape(4, 2) - fr.corners[j]).max() for j in js) < 2.0


@pytest.mark.parametrize("size", [(1920, 1080), (640, 480), (320, 240), (160, 120)])
def test_host_made_tables_equal_the_references(size):
    """The tables the product makes on the host (fid_stag_host_tables: no device needed) against the reference's own NFALUT,
    ComputeMinLineLength and Stag::fillCodeLocations; past the table's end, against nfa() itself.  Where oracle/_ref is not
    built, against the reference's tables as committed (tests/golden/stag_host_tables.npz, tools/make_stag_tables_golden.py:
    past the table's end, the least k with nfa(n, k) >= 0), which are checked against oracle/_ref wherever it is built."""
    import ctypes as C
    from fiducials_amd import _lib
    w, h = size
    L = _lib.load()
    kmin = np.zeros(4 * (w + h) + 64, np.int32)
    n, ls, mll = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    locs = np.zeros((72, 3))
    rc = L.fid_stag_host_tables(w, h, kmin.ctypes.data, len(kmin), C.byref(n), C.byref(ls), locs.ctypes.data, C.byref(mll))
    assert rc == _lib.FID_OK
    gold = np.load(os.path.join(GOLD, "stag_host_tables.npz"))
    glut, gmll, glocs, gkmin = (gold[f"{w}x{h}_{k}"] for k in ("lut", "mll", "locs", "kmin"))
    live = stag_ref.available()
    if live:
        lut, rmll, rlocs = stag_ref.host_tables(w, h)
        assert np.array_equal(lut, glut) and rmll == int(gmll) and np.array_equal(rlocs, glocs)  # the committed tables are the reference's
    else:
        lut, rmll, rlocs = glut, int(gmll), glocs
    assert n.value - len(lut) <= len(gkmin)
    assert ls.value == len(lut) == (w + h) // 8 and mll.value == rmll
    assert np.array_equal(kmin[:len(lut)], lut)
    assert np.array_equal(locs, rlocs), np.abs(locs - rlocs).max()
    for nn in list(range(len(lut), min(n.value, len(lut) + 40))) + list(range(n.value - 5, n.value)):  # k >= kmin[n]  <=>  nfa(n, k) >= 0
        km = int(kmin[nn])
        assert (km if km <= nn else nn + 1) == int(gkmin[nn - len(lut)]), nn
        if not live:
            continue
        if km <= nn:
            assert stag_ref.nfa_valid(nn, km, w, h) and (km == 0 or not stag_ref.nfa_valid(nn, km - 1, w, h)), nn
        else:
            assert not stag_ref.nfa_valid(nn, nn, w, h), nn


def test_reference_fixture_pdf_pages_read_back_their_printed_labels():
    """The reference's ONLY STag ground truth: stag_detect/test/test.pdf, 15 HD11 rasters with printed labels 00000...00014
    (tests/golden/stag_hd11_pdf.npz, tools/make_stag_golden.py).  The reference's own detector
    (oracle/_ref) with the shipped launch parameters (libraryHD 11, errorCorrection 2: stag_detect.launch:9) must read the
    printed label off every page, and reproduce the output that was committed with the fixture."""
    _need_ref()
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "stag_hd11_pdf.npz"))
    hd, ec = int(z["library_hd"]), int(z["error_correction"])
    assert (hd, ec) == (11, 2)
    for page in range(15):
        m = stag_ref.detect_markers(z["gray"][page], hd, ec)
        assert m.shape[0] == 1 and int(m[0, 0]) == int(z["labels"][page]) == page
        assert np.array_equal(m[0], z["ref_markers"][page])
        # the page is a 1000 x 1000 raster of the marker with a 10 % quiet zone: corners near (100, 100) ... (900, 900)
        assert np.abs(m[0, 1:9] - np.array([100, 100, 900, 100, 900, 900, 100, 900])).max() < 1.0
