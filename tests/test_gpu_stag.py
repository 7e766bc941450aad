"""STag EDPF front end on the MI355X, through the C-ABI, against the REFERENCE's own code
compiled in place (oracle/_ref/libstag_ref.so: ComputeGradientMapByPrewitt, ComputeAnchorPoints,
SortAnchorsByGradValue) -- integer work, bit-exact.  The 5x5 Gaussian in front is OpenCV's (not in this image): checked
against the restatement in oracle/stag_ref.cpp ("parity unpinned" for that one function)."""
import hashlib
import os

import numpy as np
import pytest

from fiducials_amd import stag as fstag
from oracle import stag_ref

pytestmark = pytest.mark.gpu

REF_OUTPUTS = os.path.join(os.path.dirname(__file__), "golden", "stag_ref_outputs.npz")
UNREFINED_CASES = [(21, 7, (1920, 1080), 20, 7), (21, 7, (640, 480), 6, 8), (11, 2, (1920, 1080), 20, 9), (15, 7, (1280, 720), 12, 10),
                   (23, 11, (800, 600), 6, 11), (19, 9, (1920, 1080), 20, 12), (13, 6, (1280, 720), 12, 13), (17, 8, (1280, 720), 12, 14)]
REFINED_CASES = [(21, 7, (1920, 1080), 20, 7), (21, 7, (640, 480), 6, 8), (11, 2, (1920, 1080), 20, 9), (15, 7, (1280, 720), 12, 10),
                 (13, 6, (1280, 720), 12, 13), (17, 8, (1280, 720), 12, 14), (19, 9, (1280, 720), 12, 15), (23, 11, (800, 600), 6, 11)]


def ref_key(call, img, *args):
    return "_".join([call, hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()[:24]] + [str(a) for a in args])


def _reference(call, img, *args):
    """stag_ref.<call>(img, *args): the reference's own code (oracle/_ref) where it is built, else what it returned for this very
    image, committed (tests/golden/stag_ref_outputs.npz, tools/make_stag_ref_outputs.py; found by the image's SHA-256).  Where
    both exist they must be equal.  A tuple result is stored as <key>#0, <key>#1, ..."""
    gold = np.load(REF_OUTPUTS)
    key = ref_key(call, img, *args)
    parts = sorted((k for k in gold.files if k.startswith(key + "#")), key=lambda k: int(k.split("#")[1]))
    assert key in gold.files or parts, f"no committed reference output for this image ({key}): rerun tools/make_stag_ref_outputs.py"
    want = gold[key] if key in gold.files else tuple(gold[k] for k in parts)
    if not stag_ref.available():
        return want
    got = getattr(stag_ref, call)(img, *args)
    same = np.array_equal(got, want) if key in gold.files else len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert same, "the committed reference output is not the reference's"
    return got


def _ref_markers(img, hd, ec, refine=True):
    return _reference("detect_markers", img, hd, ec, refine)


def _stag_like_frame(w, h, seed):
    """Dark squares with a white disc and dark code dots on a noisy gradient background (Appendix C geometry, roughly)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 140 + 40 * np.sin(xx / 97.0) * np.cos(yy / 61.0) + rng.normal(0, 3, (h, w))
    for _ in range(6):
        lo = max(4, min(40, min(w, h) // 4))
        s = int(rng.integers(lo, max(lo + 1, min(w, h) // 2)))
        x0, y0 = int(rng.integers(0, w - s)), int(rng.integers(0, h - s))
        img[y0:y0 + s, x0:x0 + s] = 25
        cy, cx, r = y0 + s / 2, x0 + s / 2, 0.4 * s
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        img[disc] = 230
        for _ in range(12):
            a, rr = rng.random() * 2 * np.pi, rng.random() * 0.7 * r
            dot = (yy - (cy + rr * np.sin(a))) ** 2 + (xx - (cx + rr * np.cos(a))) ** 2 < (0.09 * s) ** 2
            img[dot] = 30
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("size", [(640, 480), (1920, 1080), (333, 127), (64, 17)])
def test_edge_frontend_matches_reference_code(size):
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    w, h = size
    img = _stag_like_frame(w, h, seed=w * 31 + h)
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        det.edge_frontend(img)
        sm = det.tap(fstag.TAP_SMOOTH)
        assert np.array_equal(sm, stag_ref.smooth5(img)), "5x5 Gaussian (restated OpenCV fixed-point kernel)"
        # from here on the checker is the reference's own compiled code, fed with the same smoothed image
        grad, dirs = stag_ref.gradient(sm, 16)
        assert np.array_equal(det.tap(fstag.TAP_GRAD), grad)
        assert np.array_equal(det.tap(fstag.TAP_DIR), dirs)
        edge, order = stag_ref.anchors(grad, dirs, 16, 0, 1)
        assert np.array_equal(det.tap(fstag.TAP_ANCHORS), edge)
        got = det.tap(fstag.TAP_SORTED)
        assert len(got) == len(order) and len(order) > 0
        assert np.array_equal(got, order), "anchor order (ascending gradient, descending offset inside a gradient value)"
    finally:
        det.close()


def _compare_all(img, max_w=1920, max_h=1080):
    det = fstag.StagDetector(21, 7, max_width=max_w, max_height=max_h)
    try:
        det.edge_frontend(img)
        sm = det.tap(fstag.TAP_SMOOTH)
        assert np.array_equal(sm, stag_ref.smooth5(img))
        grad, dirs = stag_ref.gradient(sm, 16)
        assert np.array_equal(det.tap(fstag.TAP_GRAD), grad)
        assert np.array_equal(det.tap(fstag.TAP_DIR), dirs)
        edge, order = stag_ref.anchors(grad, dirs, 16, 0, 1)
        assert np.array_equal(det.tap(fstag.TAP_ANCHORS), edge)
        got = det.tap(fstag.TAP_SORTED)
        assert len(got) == len(order)
        assert np.array_equal(got, order)
        return len(order)
    finally:
        det.close()


@pytest.mark.parametrize("kind", ["hstripes", "vstripes", "checker", "noise", "saturated"])
def test_anchor_order_worst_cases(kind):
    """Noise-free patterns put thousands of anchors with ONE gradient value into a row (the placement's worst case:
    every lane of a wave in the same bucket), noise gives 64 different values per wave, black/white steps reach the
    largest gradient value (1530)."""
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    w, h = 1283, 517
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "hstripes":
        img = np.where((yy // 9) % 2 == 0, 40, 200)
    elif kind == "vstripes":
        img = np.where((xx // 7) % 2 == 0, 60, 180)
    elif kind == "checker":
        img = np.where(((xx // 11) + (yy // 13)) % 2 == 0, 0, 255)
    elif kind == "noise":
        img = np.random.default_rng(5).integers(0, 256, (h, w))
    else:
        img = np.where(((xx // 3) + (yy // 3)) % 2 == 0, 0, 255)
    n = _compare_all(img.astype(np.uint8))
    assert n > 1000


def _textured(w, h, seed):
    """Smooth random texture: many branching, touching edges (the routing's chain trees get deep)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, (h // 8 + 3, w // 8 + 3))
    a = np.kron(a, np.ones((8, 8)))[:h, :w]
    k = np.array([1, 4, 6, 4, 1], float) / 16
    for _ in range(3):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, a)
        a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, a)
    a = (a - a.min()) / (a.max() - a.min())
    return (255 * (np.sin(a * 40) * 0.5 + 0.5)).astype(np.uint8)


ROUTE_CASES = {
    "markers_640": lambda: _stag_like_frame(640, 480, 11),
    "markers_1080p": lambda: _stag_like_frame(1920, 1080, 12),
    "markers_odd": lambda: _stag_like_frame(333, 127, 13),
    "texture": lambda: _textured(400, 300, 14),
    "checker": lambda: np.where(((np.mgrid[0:240, 0:320][1] // 11) + (np.mgrid[0:240, 0:320][0] // 13)) % 2 == 0, 20, 235).astype(np.uint8),
    "noise": lambda: np.random.default_rng(15).integers(0, 256, (120, 160)).astype(np.uint8),
}


ROUTE_CASES["tilted_many"] = lambda: _tilted_markers(1280, 960, 34, n=48)
ROUTE_CASES["stag_1080p"] = lambda: __import__("fiducials_amd.synth", fromlist=["x"]).make_stag_frame(fstag.load_library(21), 7, 1920, 1080, 20).image
ROUTE_CASES["faint"] = lambda: _faint(480, 360, 21)


@pytest.mark.parametrize("mode", ["par", "blocks", "blocks_off", "notile", "seq"])
@pytest.mark.parametrize("case", sorted(ROUTE_CASES))
def test_edge_routing_matches_reference_code(case, mode, monkeypatch):
    """Row s4: JoinAnchorPointsUsingSortedAnchors.  Edge image and every segment (pixel by pixel, in order) against the
    reference's own routine fed with the same gradient / direction / anchor maps; the roads of the device code: one wave per
    connected component of the gradient map (default: on a dense LDS tile where the component's box fits, on 4 x 4 blocks in LDS
    where it does not; "blocks": 8 KB of LDS, so that nearly every component takes the blocks or, where even those do not fit,
    global memory; "blocks_off": the same without blocks; "notile": global memory throughout) and one lane per frame."""
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    monkeypatch.setenv("FID_STAG_ROUTE", "par" if mode.startswith("blocks") else mode)
    if mode.startswith("blocks"):
        monkeypatch.setenv("FID_STAG_TILE_KB", "8")
        if mode == "blocks_off":
            monkeypatch.setenv("FID_STAG_SPARSE", "0")
    img = ROUTE_CASES[case]()
    h, w = img.shape
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        det.detect_edges(img)
        grad, dirs, anch = det.tap(fstag.TAP_GRAD), det.tap(fstag.TAP_DIR), det.tap(fstag.TAP_ANCHORS)
        ref_edge, ref_segs = stag_ref.route(grad, dirs, anch)
        assert np.array_equal(det.tap(fstag.TAP_EDGEIMG), ref_edge)
        segs = det.edge_segments()
        assert len(segs) == len(ref_segs) and len(ref_segs) > 0
        for i, (a, b) in enumerate(zip(segs, ref_segs)):
            assert np.array_equal(a, b), f"segment {i}"
    finally:
        det.close()


def _faint(w, h, seed):
    """Low-contrast blobs on noise: most segments fail the Helmholtz test somewhere and get cut."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 120 + rng.normal(0, 6, (h, w))
    for _ in range(25):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(8, 60)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += rng.integers(-28, 28)
    k = np.array([1, 2, 1], float) / 4
    img = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, img)
    img = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, img)
    return np.clip(img, 0, 255).astype(np.uint8)


VALID_CASES = dict(ROUTE_CASES)
VALID_CASES["faint"] = lambda: _faint(480, 360, 21)
VALID_CASES["faint_big"] = lambda: _faint(1280, 720, 22)


@pytest.mark.parametrize("case", sorted(VALID_CASES))
def test_segment_validation_matches_reference_code(case):
    """Row s5: ValidateEdgeSegments.  Validated edge image and segment list against the reference's own routine fed with the
    device's EdgeMap and second smoothed image (the 3x3 blur itself is checked against its restatement)."""
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    img = VALID_CASES[case]()
    h, w = img.shape
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        det.detect_edges_validated(img)
        s2 = det.tap(fstag.TAP_SMOOTH2)
        assert np.array_equal(s2, stag_ref.smooth3(img)), "3x3 Gaussian (restated OpenCV fixed-point kernel)"
        vg = det.tap(fstag.TAP_VGRAD).astype(np.int64)
        inner = vg[1:-1, 1:-1].ravel()
        cnt = np.bincount(inner, minlength=1536)
        prob = np.cumsum(cnt[::-1])[::-1] / float((w - 2) * (h - 2))
        assert np.array_equal(det.tap(fstag.TAP_VPROB), prob), "H[g]"
        segs, pix = det.tap(fstag.TAP_SEGMENTS).reshape(-1, 2), det.tap(fstag.TAP_SEGPIX).reshape(-1, 2)
        ref_edge, ref_vsegs = stag_ref.validate(s2, pix, segs)
        assert np.array_equal(det.tap(fstag.TAP_EDGEIMG), ref_edge)
        assert np.array_equal(det.tap(fstag.TAP_VSEGMENTS).reshape(-1, 2), ref_vsegs)
        if case.startswith("faint"):
            assert len(ref_vsegs) != len(segs) or not np.array_equal(ref_vsegs, segs), "the case must exercise the cutting"
    finally:
        det.close()


def _lines_as_table(L):
    return np.stack([L[f].astype(np.float64) for f in stag_ref.LINE_FIELDS], axis=1) if len(L) else np.zeros((0, 10))


@pytest.mark.parametrize("road", ["lds", "lds64", "global"])
@pytest.mark.parametrize("case", sorted(VALID_CASES))
def test_line_fitting_matches_reference_code(case, road, monkeypatch):
    """Row s6, first half: SplitSegment2Lines + JoinCollinearLines.  Every field of every line bit for bit (doubles compared
    with ==) against the reference's own routines fed with the device's validated EdgeMap; the segment's pixels and prefix sums
    in LDS (default: up to 1 024 pixels), with only 64 pixels of LDS per wave (nearly every segment in global memory, the short
    ones in LDS side by side) and in global memory throughout."""
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    if road != "lds":
        monkeypatch.setenv("FID_STAG_SPLIT_LDS", "64" if road == "lds64" else "0")
    img = VALID_CASES[case]()
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        det.detect_lines(img)
        vsegs, pix = det.tap(fstag.TAP_VSEGMENTS).reshape(-1, 2), det.tap(fstag.TAP_SEGPIX).reshape(-1, 2)
        ref, mll = stag_ref.fit_lines(img, pix, vsegs, validate=False)
        got = _lines_as_table(det.lines())
        assert got.shape == ref.shape, (got.shape, ref.shape)
        bad = np.nonzero(~(got == ref).all(axis=1))[0]
        assert len(bad) == 0, (bad[:5], got[bad[:2]], ref[bad[:2]])
        if case.startswith(("markers", "faint", "texture")):
            assert len(ref) > 0
    finally:
        det.close()


@pytest.mark.parametrize("case", sorted(VALID_CASES))
def test_detect_lines_end_to_end_matches_reference(case):
    """Rows s2-s6 together = EDInterface::runEDPFandEDLines: the device pipeline from the raw image against the reference's
    DetectLinesByEDPF run end to end (oracle/_ref; only SmoothImage restated): validated segments and final lines."""
    img = VALID_CASES[case]()
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        det.detect_lines_validated(img)
        ref_lines, ref_segs, ref_pix = _reference("detect_lines", img)
        vsegs, pix = det.tap(fstag.TAP_VSEGMENTS).reshape(-1, 2), det.tap(fstag.TAP_SEGPIX).reshape(-1, 2)
        assert np.array_equal(vsegs, ref_segs)
        for a, n in ref_segs:
            assert np.array_equal(pix[a:a + n], ref_pix[a:a + n])
        got = _lines_as_table(det.lines(validated=True))
        assert got.shape == ref_lines.shape, (got.shape, ref_lines.shape)
        assert (got == ref_lines).all()
        before = len(det.lines())
        if case.startswith("faint"):
            assert len(ref_lines) < before, "the case must exercise the rejection"
    finally:
        det.close()


def _tilted_markers(w, h, seed, n=10):
    """Dark quadrilaterals (rotated, perspective-like) with a white disc inside, one per cell of a grid, on a light noisy
    background."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 190 + 20 * np.sin(xx / 131.0) + rng.normal(0, 2, (h, w))
    gx = int(np.ceil(np.sqrt(n * w / h)))
    gy = int(np.ceil(n / gx))
    cw, chh = w / gx, h / gy
    for k in range(n):
        s = rng.uniform(0.2, 0.3) * min(cw, chh)
        cx, cy = (k % gx + 0.5) * cw + rng.uniform(-0.1, 0.1) * cw, (k // gx + 0.5) * chh + rng.uniform(-0.1, 0.1) * chh
        ang = rng.uniform(0, 2 * np.pi)
        base = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float) * s
        base += rng.uniform(-0.12, 0.12, (4, 2)) * s  # perspective-like distortion
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        P = base @ R.T + [cx, cy]
        inside = np.ones((h, w), bool)
        for i in range(4):
            a, b = P[i], P[(i + 1) % 4]
            inside &= (b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0]) >= 0
        img[inside] = 30
        img[(xx - cx) ** 2 + (yy - cy) ** 2 < (0.4 * s) ** 2] = 225
    k3 = np.array([1, 2, 1], float) / 4
    img = np.apply_along_axis(lambda v: np.convolve(v, k3, mode="same"), 0, img)
    img = np.apply_along_axis(lambda v: np.convolve(v, k3, mode="same"), 1, img)
    return np.clip(img, 0, 255).astype(np.uint8)


QUAD_CASES = dict(VALID_CASES)
QUAD_CASES["tilted_640"] = lambda: _tilted_markers(640, 480, 31)
QUAD_CASES["tilted_1080p"] = lambda: _tilted_markers(1920, 1080, 32, n=20)
QUAD_CASES["tilted_small"] = lambda: _tilted_markers(320, 240, 33, n=4)
QUAD_CASES["tilted_many"] = lambda: _tilted_markers(1280, 960, 34, n=48)


def _quads_as_table(Q):
    if not len(Q):
        return np.zeros((0, 12))
    return np.concatenate([Q["corners"].reshape(-1, 8), Q["lineInf"], Q["projectiveDistortion"][:, None]], axis=1)


@pytest.mark.parametrize("case", sorted(QUAD_CASES))
def test_quads_match_reference_code(case):
    """Row s7: QuadDetector::detectQuads from the raw image, against the reference's own QuadDetector / Quad / EDInterface
    sources compiled in place (oracle/cvshim supplies the cv:: data types only): corners, vanishing line and projective
    distortion of every quad, doubles compared with ==."""
    img = QUAD_CASES[case]()
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        det.detect_quads(img)
        ref, _ = _reference("detect_quads", img)
        got = _quads_as_table(det.quads())
        assert got.shape == ref.shape, (got.shape, ref.shape)
        assert (got == ref).all(), (got[~(got == ref).all(axis=1)][:2], ref[~(got == ref).all(axis=1)][:2])
        if case.startswith(("tilted", "markers_6", "markers_1")):
            assert len(ref) > 0
    finally:
        det.close()


def _markers_as_table(M):
    if not len(M):
        return np.zeros((0, 24))
    return np.concatenate([M["id"][:, None].astype(np.float64), M["corners"].reshape(-1, 8), M["center"], M["H"].reshape(-1, 9), M["lineInf"],
                           M["projectiveDistortion"][:, None]], axis=1)


@pytest.mark.parametrize("hd,ec,size,n,seed", UNREFINED_CASES)
def test_markers_unrefined_match_reference_code(hd, ec, size, n, seed):
    """Row s8 (+ s1's loop): homography, code reading, decoding, corner shift, duplicate removal on rendered STag markers,
    against the reference's own Stag.cpp / Decoder.cpp / Marker.cpp compiled in place (pose refinement switched off on both
    sides; the Otsu threshold behind cv::threshold is restated in the oracle): ids exact, all doubles compared with ==."""
    from fiducials_amd import synth
    w, h = size
    words = fstag.load_library(hd)
    fr = synth.make_stag_frame(words, seed, w, h, n)
    det = fstag.StagDetector(hd, ec, max_width=1920, max_height=1080)
    try:
        det.detect_markers_unrefined(fr.image)
        M = det.markers()
        ref = _ref_markers(fr.image, hd, ec, refine=False)
        assert len(ref) >= min(n, len(words) // 4) // 2, "the rendered markers must be readable"
        got = _markers_as_table(M)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        assert np.array_equal(got[:, 0], ref[:, 0]), "ids"
        assert (got == ref).all(), np.abs(got - ref).max(axis=0)
        assert set(M["id"].tolist()) <= set(fr.ids.tolist())
    finally:
        det.close()


@pytest.mark.parametrize("hd,ec,size,n,seed", REFINED_CASES)
def test_detect_markers_refined_matches_reference(hd, ec, size, n, seed):
    """Rows s1 + s9 = Stag::detectMarkers complete.  The refinement runs a Nelder-Mead search whose cost calls atan / sin /
    cos: the device's math library and glibc agree to rounding only, so this row is held to a tolerance: ids exact, corners
    and centre within 1e-3 px of the reference's (PoseRefiner.cpp + Ellipse.cpp compiled in place; cv::DownhillSolver and
    the 3 x 3 inverse restated on the checker's side as well -- parity unpinned for those two)."""
    from fiducials_amd import synth
    w, h = size
    words = fstag.load_library(hd)
    fr = synth.make_stag_frame(words, seed, w, h, n)
    det = fstag.StagDetector(hd, ec, max_width=1920, max_height=1080)
    try:
        M = det.detect_markers(fr.image)
        ref = _ref_markers(fr.image, hd, ec, refine=True)
        unref = _ref_markers(fr.image, hd, ec, refine=False)
        assert len(M) == len(ref) > 0
        assert np.array_equal(M["id"], ref[:, 0].astype(np.int32))
        dc = np.abs(M["corners"].reshape(-1, 8) - ref[:, 1:9]).max()
        dz = np.abs(M["center"] - ref[:, 9:11]).max()
        moved = np.abs(ref[:, 1:9] - unref[:, 1:9]).max()
        assert moved > 1e-2, "the refinement must have done something in this case"
        assert dc < 1e-3 and dz < 1e-3, (dc, dz)
        # and it lands on the rendered geometry: refined corners within 2 px of the generator's ground truth
        for k in range(len(M)):
            cand = [np.abs(M["corners"][k] - fr.corners[j]).max() for j in np.flatnonzero(fr.ids == M["id"][k])]
            assert min(cand) < 2.0, (k, cand)
    finally:
        det.close()


def test_reference_fixture_pdf_pages_on_the_device():
    """The reference's only STag fixtures (stag_detect/test/test.pdf: 15 HD11 rasters, printed labels 00000...00014;
    tests/golden/stag_hd11_pdf.npz) through fid_stag_detect_markers with the shipped launch parameters (libraryHD 11,
    errorCorrection 2, stag_detect.launch:9): the id read on the device == the label printed on the page == what the
    reference's own detector returns (oracle/_ref when built, else the output committed with the fixture), corners and centre
    within the refined path's stated 1e-3 px."""
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "stag_hd11_pdf.npz"))
    det = fstag.StagDetector(11, 2, max_width=1000, max_height=1000)
    try:
        for page in range(15):
            M = det.detect_markers(z["gray"][page])
            ref = stag_ref.detect_markers(z["gray"][page], 11, 2) if stag_ref.available() else z["ref_markers"][page][None, :]
            assert np.array_equal(ref[0], z["ref_markers"][page])
            assert len(M) == 1 and int(M["id"][0]) == page == int(z["labels"][page]) == int(ref[0, 0])
            assert np.abs(M["corners"].reshape(-1, 8) - ref[:, 1:9]).max() < 1e-3
            assert np.abs(M["center"] - ref[:, 9:11]).max() < 1e-3
        # and the unrefined stage, where every double is compared with ==
        for page in (0, 7, 14):
            det.detect_markers_unrefined(z["gray"][page])
            got = _markers_as_table(det.markers())
            ref = _ref_markers(z["gray"][page], 11, 2, refine=False)
            assert got.shape == ref.shape and (got == ref).all()
    finally:
        det.close()


def test_the_benchmarked_cfg5_frames_equal_the_reference():
    """The frames `bench.py` times for cfg 5 (bench.make_stag_frames(shard_seeds(0, 1, 16, "stag")): 1920x1080, every id of
    library HD21 once per frame) ARE the frames compared here (round 2 timed seeds 100..103 and tested others): ids exact,
    corners and centre within the refined path's 1e-3 px of the reference's own Stag::detectMarkers (oracle/_ref), at least 10 of
    the 12 rendered ids read on every frame, and the batch entry point returns the same markers as the frame-at-a-time one."""
    import bench
    frames = bench.make_stag_frames(bench.shard_seeds(0, 1, bench.STAG_UNIQUE, "stag"))
    assert len(frames) == 16 and len({f.tobytes() for f in frames}) == 16
    det = fstag.StagDetector(bench.STAG_HD, bench.STAG_EC, max_width=1920, max_height=1080)
    found = []
    try:
        for f in frames:
            M = det.detect_markers(f)
            ref = _ref_markers(f, bench.STAG_HD, bench.STAG_EC)
            assert len(M) == len(ref) >= 10 and len(set(M["id"].tolist())) == len(M)
            assert np.array_equal(M["id"], ref[:, 0].astype(np.int32))
            assert np.abs(M["corners"].reshape(-1, 8) - ref[:, 1:9]).max() < 1e-3 and np.abs(M["center"] - ref[:, 9:11]).max() < 1e-3
            found.append(M)
    finally:
        det.close()
    pool = fstag.StagPool(bench.STAG_HD, bench.STAG_EC, n_contexts=4, max_width=1920, max_height=1080)
    try:
        from fiducials_amd import synth
        ms, _ = pool.detect_markers_batch(np.stack(frames), synth.K_DEFAULT, None, 0.18)
        for a, b in zip(ms, found):
            assert np.array_equal(a["id"], b["id"]) and np.array_equal(a["corners"], b["corners"])
        # a caller slot that is too small: FID_E_CAPACITY, and the count of such a frame is 0 (nothing was copied for it:
        # a C caller that walks n_per_frame[f] entries must not run into its neighbour's slot)
        from fiducials_amd import _lib
        cap = 4
        fr2 = np.ascontiguousarray(np.stack(frames[:2]))
        markers = np.zeros((2, cap), fstag.MARKER_DTYPE)
        poses = np.zeros((2, cap), fstag.POSE_DTYPE)
        counts = np.full(2, -1, np.int32)
        Kp, Dp = np.ascontiguousarray(synth.K_DEFAULT, dtype=np.float64).reshape(9), np.zeros(5)
        rc = pool._L.fid_stag_detect_markers_batch(pool._arr, len(pool.dets), fr2.ctypes.data, 2, 1920, 1080, 1920, 1920 * 1080, Kp.ctypes.data,
                                                   Dp.ctypes.data, 0.18, markers.ctypes.data, poses.ctypes.data, cap, counts.ctypes.data)
        assert rc == _lib.FID_E_CAPACITY and counts.tolist() == [0, 0]
    finally:
        pool.close()


def test_aruco_and_stag_contexts_share_a_process():
    """A node that hosts an aruco AND a STag detector in one process (round 2: STag throughput ran a HIP stream per frame slot
    and collapsed from 1 400 to 8 frames/s when other contexts held hardware queues).  With frames as a grid dimension the STag
    batch uses one stream per group of 16: its rate with an aruco context open (and working) beside it stays within a factor
    of its rate alone, and so does the aruco batch rate with the STag pool open; results unchanged."""
    import time
    import bench
    from fiducials_amd import synth
    from fiducials_amd.detector import ArucoDetector
    frames = np.stack(bench.make_stag_frames(bench.shard_seeds(0, 1, bench.STAG_UNIQUE, "stag")) * 2)  # 32 frames

    def stag_rate(pool):
        pool.detect_markers_batch(frames, synth.K_DEFAULT, None, 0.18)
        best, ms = 0.0, None
        for _ in range(3):
            t = time.perf_counter()
            ms, _ = pool.detect_markers_batch(frames, synth.K_DEFAULT, None, 0.18)
            best = max(best, len(frames) / (time.perf_counter() - t))
        return best, [m["id"].tolist() for m in ms]

    def aruco_rate(det, imgs):
        det.detect_markers_batch(imgs, unpack=False)
        best = 0.0
        for _ in range(3):
            t = time.perf_counter()
            n = det.detect_markers_batch(imgs, unpack=False)
            best = max(best, len(imgs) / (time.perf_counter() - t))
        return best, n

    pool = fstag.StagPool(bench.STAG_HD, bench.STAG_EC, n_contexts=32, max_width=1920, max_height=1080)
    try:
        alone, ids_alone = stag_rate(pool)
        aimgs = bench.make_frames(bench.shard_seeds(0, 1, 16))
        det = ArucoDetector(6, max_width=1920, max_height=1080, max_batch=16, max_markers=64)
        try:
            a_with, n_with = aruco_rate(det, aimgs)
            beside, ids_beside = stag_rate(pool)
            assert ids_beside == ids_alone
            assert beside > 0.5 * alone, (alone, beside)
        finally:
            det.close()
    finally:
        pool.close()
    det = ArucoDetector(6, max_width=1920, max_height=1080, max_batch=16, max_markers=64)
    try:
        a_alone, n_alone = aruco_rate(det, aimgs)
    finally:
        det.close()
    assert n_with == n_alone == [20] * 16
    assert a_with > 0.5 * a_alone, (a_alone, a_with)


def test_marker_pose_matches_oracle():
    """Row s10: Common::solvePnpSingle on centre + four corners (5 coplanar points), against the oracle's restatement of
    cv::solvePnP(ITERATIVE) fed with the same markers: rotation matrix / tvec to 1e-6, and against the generator's pose to 2 %.
    The device starts its Levenberg-Marquardt from a closed-form 4-corner pose, the oracle from the 5-point DLT.  That the two
    end in the same minimum is a property of these problems, not of the algorithm: test_gpu_pose_sweep.py found it true (2.1e-7
    at worst) for every detected marker under 14 cameras whose five points some pose explains to 4 px rms, this camera among
    them, and false (up to 1.4e-2 in R) for the few that none does, where the 20-iteration cap ends both runs in a flat valley."""
    import oracle
    from fiducials_amd import synth
    words = fstag.load_library(21)
    fr = synth.make_stag_frame(words, 7, 1920, 1080, 20)
    K = np.array([[1400.0, 0, 960.0], [0, 1400.0, 540.0], [0, 0, 1]])
    D = np.array([0.05, -0.02, 0.001, -0.0005, 0.0])
    size = synth.MARKER_LEN
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        M = det.detect_markers(fr.image)
        assert len(M) >= 6
        for Dv in (np.zeros(5), D):
            P = det.pose_last(K, Dv, size)
            assert np.array_equal(P["id"], M["id"])
            h = float(np.float32(size / 2.0))
            obj = np.array([[0, 0, 0], [-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0]], float)
            for k in range(len(M)):
                img = np.concatenate([M["center"][k][None, :], M["corners"][k]], axis=0)
                r, t = oracle.solve_pnp_points(K, Dv, obj, img)
                # the node uses the rotation MATRIX (common.hpp:43); near a half turn the same rotation has two vectors
                assert np.abs(P["R"][k] - synth._rodrigues(r)).max() < 1e-6 and np.abs(P["tvec"][k] - t).max() < 1e-6, (k, P["rvec"][k], r)
                assert np.abs(P["R"][k] - synth._rodrigues(P["rvec"][k])).max() < 1e-12
        P = det.pose_last(K, np.zeros(5), size)
        for k in range(len(M)):  # the rendered distance (several markers may share an id: the nearest one counts)
            cand = [np.linalg.norm(P["tvec"][k] - fr.tvecs[j]) / np.linalg.norm(fr.tvecs[j]) for j in np.flatnonzero(fr.ids == M["id"][k])]
            assert min(cand) < 0.02, (k, cand)
    finally:
        det.close()


def test_empty_and_degenerate_frames_go_through_every_stage():
    """Nothing to find is a result, not an error: a flat frame (no anchors), a tiny frame, a frame of pure noise at 640x480
    (one gradient component holding nearly every anchor: the routing's worst case for parallelism) -- all through
    fid_stag_detect_markers, the noise frame's edge map and lines checked against the reference."""
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        for img in (np.full((480, 640), 90, np.uint8), np.full((17, 64), 200, np.uint8)):
            assert len(det.detect_markers(img)) == 0
            assert len(det.tap(fstag.TAP_SORTED)) == 0 and len(det.edge_segments()) == 0 and len(det.lines(validated=True)) == 0
            assert len(det.quads()) == 0
            assert len(det.pose_last(np.eye(3), None, 0.18)) == 0
        noise = np.random.default_rng(41).integers(0, 256, (480, 640)).astype(np.uint8)
        assert len(det.detect_markers(noise)) == 0
        ref_lines, ref_segs, ref_pix = stag_ref.detect_lines(noise)
        vsegs, pix = det.tap(fstag.TAP_VSEGMENTS).reshape(-1, 2), det.tap(fstag.TAP_SEGPIX).reshape(-1, 2)
        assert np.array_equal(vsegs, ref_segs)  # (the Helmholtz test throws noise away: possibly nothing is left)
        _, raw = stag_ref.route(det.tap(fstag.TAP_GRAD), det.tap(fstag.TAP_DIR), det.tap(fstag.TAP_ANCHORS))
        mine = det.edge_segments()
        assert len(raw) > 1000 and len(mine) == len(raw) and all(np.array_equal(a, b) for a, b in zip(mine, raw))
        for a, n in ref_segs:
            assert np.array_equal(pix[a:a + n], ref_pix[a:a + n])
        # (the lines tap holds the direction-corrected lines after the quad stage: compare the untouched fields)
        got = _lines_as_table(det.lines(validated=True))
        assert got.shape == ref_lines.shape
        assert np.array_equal(got[:, [0, 1, 6, 7, 8, 9]], ref_lines[:, [0, 1, 6, 7, 8, 9]])
    finally:
        det.close()


def test_noise_at_720p_takes_the_sequential_road_and_still_matches():
    """A 1280x720 frame of pure noise: one gradient component with hundreds of thousands of anchors.  The component-parallel
    road declines (nothing to run side by side), the call repeats on the sequential road; edge image and segments as the
    reference's, in bounded time."""
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    import time
    noise = np.random.default_rng(43).integers(0, 256, (720, 1280)).astype(np.uint8)
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    try:
        t0 = time.perf_counter()
        det.detect_edges(noise)
        dt = time.perf_counter() - t0
        ref_edge, raw = stag_ref.route(det.tap(fstag.TAP_GRAD), det.tap(fstag.TAP_DIR), det.tap(fstag.TAP_ANCHORS))
        assert np.array_equal(det.tap(fstag.TAP_EDGEIMG), ref_edge)
        mine = det.edge_segments()
        assert len(mine) == len(raw) > 5000 and all(np.array_equal(a, b) for a, b in zip(mine, raw))
        assert dt < 20.0, dt
        print(f"720p noise: {len(det.tap(fstag.TAP_SORTED))} anchors, {len(raw)} segments, {dt * 1e3:.0f} ms")
    finally:
        det.close()


def test_batch_entry_point_equals_frame_by_frame():
    """fid_stag_detect_markers_batch (frames spread over several contexts and host threads inside the library) returns, frame
    for frame, what fid_stag_detect_markers + fid_stag_pose_last return on one context."""
    from fiducials_amd import synth
    words = fstag.load_library(21)
    frames = np.stack([synth.make_stag_frame(words, 50 + i, 1280, 720, 8).image for i in range(5)] * 2)
    K = np.array([[933.3, 0, 640.0], [0, 933.3, 360.0], [0, 0, 1]])
    pool = fstag.StagPool(21, 7, n_contexts=4, max_width=1280, max_height=720)
    det = fstag.StagDetector(21, 7, max_width=1280, max_height=720)
    try:
        M, P = pool.detect_markers_batch(frames, K, None, 0.18)
        assert len(M) == len(frames)
        for f in range(len(frames)):
            m = det.detect_markers(frames[f])
            p = det.pose_last(K, None, 0.18)
            assert len(m) >= 3 and m.tobytes() == M[f].tobytes() and p.tobytes() == P[f].tobytes(), f
    finally:
        pool.close()
        det.close()


def test_a_frame_refused_in_the_routing_leaves_no_stage_of_the_frame_before_readable(monkeypatch):
    """A walk of more than 32 767 chains from one anchor is refused (FID_E_CAPACITY; the reference's short chain indices would
    wrap there, EDInternals.cpp:39-45) -- frames of uniform noise can get there.  The frame before must not shine through: no
    markers in the tap, fid_stag_pose_last refuses, the Python host raises; the next frame is served as if nothing had happened;
    same on the counted road and queued ahead (found by tools/gpu_stag_spec_stress.py, seed 11)."""
    from fiducials_amd import synth, _lib
    from fiducials_amd._lib import FidError
    words = fstag.load_library(21)
    w, h = 1280, 720
    good = synth.make_stag_frame(words, 300, w, h, 5).image
    K = np.array([[933.3, 0, 640.0], [0, 933.3, 360.0], [0, 0, 1]])
    det = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    try:
        noise = None
        for seed in range(24):
            f = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
            try:
                det.detect_edges(f)
            except FidError as e:
                assert e.status == _lib.FID_E_CAPACITY
                noise = f
                break
    finally:
        det.close()
    if noise is None:
        pytest.skip("no noise frame among the seeds reaches the chain limit")
    for road in ("0", "1"):
        monkeypatch.setenv("FID_STAG_SPEC", road)
        det = fstag.StagDetector(21, 7, max_width=w, max_height=h)
        try:
            want = det.detect_markers(good)
            assert len(want) >= 3
            pose = det.pose_last(K, None, 0.18)
            with pytest.raises(FidError) as ei:
                det.detect_markers(noise)
            assert ei.value.status == _lib.FID_E_CAPACITY
            assert len(det.markers()) == 0 and len(det.quads()) == 0
            with pytest.raises(FidError):
                det.pose_last(K, None, 0.18)
            again = det.detect_markers(good)
            assert again.tobytes() == want.tobytes() and det.pose_last(K, None, 0.18).tobytes() == pose.tobytes()
        finally:
            det.close()


def test_frames_queued_ahead_equal_the_counted_road(monkeypatch):
    """Round 5: a context that has finished a frame sizes the next frame's launches by that frame's counts and enqueues the whole
    frame without the nine host waits (fid_stag.hip, stag_advance_impl); a frame whose counts outgrow the sizes is caught by
    k_stag_spec_guard / the host check at the frame's one wait and run again on the counted road.  Same bytes either way: a
    sequence that goes from few markers to many (a miss), back (a fit), through an empty frame and a staged call, against
    FID_STAG_SPEC=0 on a context of its own; poses too; and the batch entry point with slots that remember their last frame."""
    from fiducials_amd import synth
    words = fstag.load_library(21)
    w, h = 1280, 720
    small = [synth.make_stag_frame(words, 300 + i, w, h, 2).image for i in range(2)]
    big = [synth.make_stag_frame(words, 310 + i, w, h, 12).image for i in range(2)]
    blank = np.full((h, w), 128, np.uint8)
    seq = [small[0], small[1], small[0], big[0], big[1], big[0], small[0], blank, big[1], small[1], small[1]]
    K = np.array([[933.3, 0, 640.0], [0, 933.3, 360.0], [0, 0, 1]])
    monkeypatch.setenv("FID_STAG_SPEC", "0")
    det0 = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    want = []
    try:
        for f in seq:
            m = det0.detect_markers(f)
            want.append((m.tobytes(), det0.pose_last(K, None, 0.18).tobytes(), len(m)))
        assert det0.queue_stats() == (0, 0)
    finally:
        det0.close()
    assert want[3][2] >= 8 and want[0][2] >= 1 and want[7][2] == 0
    monkeypatch.setenv("FID_STAG_SPEC", "1")
    det1 = fstag.StagDetector(21, 7, max_width=w, max_height=h)
    try:
        for k, f in enumerate(seq):
            m = det1.detect_markers(f)
            assert (m.tobytes(), det1.pose_last(K, None, 0.18).tobytes(), len(m)) == want[k], k
            if k == 4:  # a staged call in between takes the counted road and leaves the context usable
                det1.detect_quads(big[0])
                assert len(det1.quads()) > 0
        queued, rerun = det1.queue_stats()
        assert queued >= 6 and 1 <= rerun < queued, (queued, rerun)  # (small -> big and the empty frame are misses, the rest fit)
        # the stage taps after a frame that was queued ahead are those of the counted road (the host-side counts were taken over)
        det1.detect_markers(big[0])
        q1 = det1.quads().tobytes()
        l1 = det1.lines(validated=True).tobytes()
        e1 = [p.tobytes() for p in det1.edge_segments(validated=True)]
        assert det1.queue_stats()[0] == queued + 1
        det1.detect_quads(big[0])
        assert det1.quads().tobytes() == q1 and det1.lines(validated=True).tobytes() == l1
        assert [p.tobytes() for p in det1.edge_segments(validated=True)] == e1
    finally:
        det1.close()
    # group mode: the second call finds every slot with the counts of its last frame
    frames = np.stack([small[0], big[0], small[1], big[1], blank, big[0], small[0], big[1]])
    idx = [0, 3, 1, 4, 7, 3, 0, 4]
    pool = fstag.StagPool(21, 7, n_contexts=4, max_width=w, max_height=h)
    try:
        for rnd in range(3):
            M, P = pool.detect_markers_batch(frames if rnd != 1 else frames[::-1], K, None, 0.18)
            order = idx if rnd != 1 else idx[::-1]
            for f in range(len(frames)):
                assert (M[f].tobytes(), P[f].tobytes(), len(M[f])) == want[order[f]], (rnd, f)
        assert sum(d.queue_stats()[0] for d in pool.dets) >= 8
    finally:
        pool.close()


def test_a_group_with_few_and_many_markers_hands_every_frame_its_own(monkeypatch):
    """Round 5, found with the frames queued ahead: the hand-over of a frame's markers is an alias KERNEL up to 4 KB and a COPY
    above, recorded at the same launch site -- a group that held both kinds issued the kernel and dropped the copies, so a frame
    with many markers returned what its slot had held before.  Frames of 2 and of 30 HD11 markers side by side in groups of two,
    on the counted road and queued ahead, against a context of their own."""
    from fiducials_amd import synth
    words = fstag.load_library(11)
    w, h = 1920, 1080
    few = [synth.make_stag_frame(words, 400 + i, w, h, 2).image for i in range(2)]
    many = [synth.make_stag_frame(words, 410 + i, w, h, 30).image for i in range(2)]
    frames = np.stack([few[0], many[0], many[1], few[1], many[0], few[0]])
    K = synth.K_DEFAULT
    monkeypatch.setenv("FID_STAG_SPEC", "0")
    det = fstag.StagDetector(11, 2, max_width=w, max_height=h)
    try:
        want = []
        for f in frames:
            m = det.detect_markers(f)
            want.append((m.tobytes(), det.pose_last(K, None, 0.18).tobytes(), len(m)))
    finally:
        det.close()
    assert want[1][2] > 24 and want[2][2] > 24 and want[0][2] <= 2  # (more than 4 KB of markers / less)
    for spec in ("0", "1"):
        monkeypatch.setenv("FID_STAG_SPEC", spec)
        pool = fstag.StagPool(11, 2, n_contexts=4, max_width=w, max_height=h)
        try:
            for rnd in range(2):
                M, P = pool.detect_markers_batch(frames, K, None, 0.18, cap_per_frame=64)
                for f in range(len(frames)):
                    assert (M[f].tobytes(), P[f].tobytes(), len(M[f])) == want[f], (spec, rnd, f)
        finally:
            pool.close()


def test_stag_status_codes():
    from fiducials_amd import _lib
    from fiducials_amd._lib import FidError
    with pytest.raises(FidError):
        fstag.StagDetector(12, 2)  # even library
    with pytest.raises(FidError):
        fstag.StagDetector(21, 11)  # errorCorrection > (HD - 1) / 2
    det = fstag.StagDetector(21, 7, max_width=320, max_height=240)
    try:
        with pytest.raises(FidError) as e:
            det.edge_frontend(np.zeros((241, 320), np.uint8))
        assert e.value.status == _lib.FID_E_INVALID_ARG
        det.edge_frontend(np.full((240, 320), 77, np.uint8))  # flat image: no anchors
        assert len(det.tap(fstag.TAP_SORTED)) == 0 and not det.tap(fstag.TAP_ANCHORS).any()
    finally:
        det.close()


def test_groups_of_32_and_contexts_of_two_sizes_equal_the_frame_at_a_time_road(monkeypatch):
    """Round 6: a group's launch carries frame 0's arguments once and, per further frame, the distance of its context's slab (and
    of its pinned block) from frame 0's -- every context carves its buffers out of one slab at the same offsets (fid_stag_batch.h,
    fid_stag_create).  (a) 64 slots = two groups of 32, 80 frames (a second, partly filled round): markers and poses of every frame
    == the frame-at-a-time road's.  (b) the same call with the contexts of a group made for TWO image sizes (their slabs are laid
    out differently, so a frame's arguments are NOT frame 0's moved by a delta): the recorder must notice and launch such frames on
    their own -- same results, nothing merged that does not fit.  (c) groups of 3 (a frame-minor launch of an odd size)."""
    import bench
    from fiducials_amd import synth

    frames = bench.make_stag_frames(bench.shard_seeds(0, 1, bench.STAG_UNIQUE, "stag"))
    batch = np.stack([frames[(5 * i) % len(frames)] for i in range(80)])
    one = fstag.StagDetector(bench.STAG_HD, bench.STAG_EC, max_width=1920, max_height=1080)
    try:
        want = []
        for f in frames:
            M = one.detect_markers(f).copy()
            P = one.pose_last(synth.K_DEFAULT, None, 0.18).copy()
            want.append((M, P))
    finally:
        one.close()

    def check(pool, imgs, idx):
        ms, ps = pool.detect_markers_batch(imgs, synth.K_DEFAULT, None, 0.18)
        assert len(ms) == len(imgs)
        for k, (m, p) in enumerate(zip(ms, ps)):
            M, P = want[idx(k)]
            assert len(m) == len(M) and len(p) == len(P), k
            for name in M.dtype.names:
                assert np.array_equal(m[name], M[name]), (k, name)
            for name in P.dtype.names:
                assert np.array_equal(p[name], P[name]), (k, name)

    pool = fstag.StagPool(bench.STAG_HD, bench.STAG_EC, n_contexts=64, max_width=1920, max_height=1080)
    try:
        check(pool, batch, lambda k: (5 * k) % len(frames))
        monkeypatch.setenv("FID_STAG_GROUP", "3")
        check(pool, batch[:17], lambda k: (5 * k) % len(frames))
        monkeypatch.delenv("FID_STAG_GROUP")
    finally:
        pool.close()
    # (b) every other context made for a larger image: another slab layout inside one group
    pool = fstag.StagPool(bench.STAG_HD, bench.STAG_EC, n_contexts=8, max_width=1920, max_height=1080)
    try:
        for k in (1, 3, 6):
            pool.dets[k].close()
            pool.dets[k] = fstag.StagDetector(bench.STAG_HD, bench.STAG_EC, 2048, 1100)
            pool._arr[k] = pool.dets[k]._ctx.value
        monkeypatch.setenv("FID_STAG_GROUP", "8")
        check(pool, batch[:24], lambda k: (5 * k) % len(frames))
    finally:
        pool.close()
