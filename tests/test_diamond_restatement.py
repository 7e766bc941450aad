"""ChArUco diamonds on the CPU: the layout and one diamond enumerated by hand, the package's CharucoDiamond against the restatement, the
whole chain restated -- oracle.detect, proposals, resolution, positions, oracle.corner_subpix -- on rendered frames against the true
projections, and the measurement behind the default of max_rep_rate.  No device."""
import numpy as np
import pytest

import diamond_cases as dc
import diamond_restatement as dr
from fiducials_amd import _lib, synth
from fiducials_amd.charuco import CharucoDiamond


def test_the_abi_names_the_entry_points():
    for name in ("fid_default_diamond_opts", "fid_diamonds_last", "fid_diamonds_detect", "fid_diamond_pose_cam"):
        assert name in _lib.SYMBOLS
    assert _lib.DIAMOND_DTYPE.itemsize == 4 * (4 + 4 + 8 + 8 + 4)
    import ctypes as C
    assert C.sizeof(_lib.FidDiamondOpts) == 24
    assert (_lib.DIAMOND_MAX_PER_FRAME, _lib.DIAMOND_MAX_MARKERS) == (dr.MAX_PER_FRAME, dr.MAX_MARKERS) == (64, 256)


def test_the_layout_against_the_enumeration():
    """L(2): markers of side 1 in squares of 2 (all exact in float), d = 0.5"""
    L = dr.layout(2.0)
    assert L.marker_obj[0].tolist() == [[2.5, 1.5, 0], [3.5, 1.5, 0], [3.5, 0.5, 0], [2.5, 0.5, 0]]  # k = 0: square (1, 0)
    assert L.marker_obj[1, 0].tolist() == [0.5, 3.5, 0] and L.marker_obj[2, 0].tolist() == [4.5, 3.5, 0]  # squares (0, 1), (2, 1)
    assert L.marker_obj[3, 0].tolist() == [2.5, 5.5, 0]  # square (1, 2)
    assert L.corner_obj.tolist() == [[2, 2, 0], [4, 2, 0], [2, 4, 0], [4, 4, 0]]
    assert L.near_marker.tolist() == [[0, 1], [0, 2], [1, 3], [2, 3]] and L.near_corner.tolist() == [[0, 2], [1, 3], [1, 3], [0, 2]]
    p = CharucoDiamond((9, 9, 4, 0), 2.0, 1.0)
    assert np.array_equal(p.marker_object_points, L.marker_obj) and np.array_equal(p.corner_object_points, L.corner_obj)
    assert np.array_equal(p.nearest_markers, L.near_marker) and np.array_equal(p.nearest_corners, L.near_corner)
    assert p.ids.tolist() == [9, 9, 4, 0] and p.square_marker_rate == 2.0 and p.centre.tolist() == [3.0, 3.0, 0.0]
    assert p.record_object_points[:, :2].tolist() == [[2, 4], [4, 4], [4, 2], [2, 2]]  # top left, top right, bottom right, bottom left


def _square(x, y, m):
    """a marker of side m px whose top-left corner is (x, y), in image coordinates (y down)"""
    return [[x, y], [x + m, y], [x + m, y + m], [x, y + m]]


def test_a_diamond_enumerated_by_hand():
    """Rate 2, markers of 40 px, squares of 80 px, the diamond's 3 x 3 board with its top-left corner at (100, 60) in the image.  The
    board's y points up: square (1, 0) is the bottom middle one.  Listed: a loose marker, then the markers of squares (1, 2), (2, 1),
    (1, 0), (0, 1) -- the anchor third."""
    m, s, x0, y0 = 40.0, 80.0, 100.0, 60.0

    def in_square(sx, sy):  # (board square, y up) -> the marker centred in it
        return _square(x0 + sx * s + (s - m) / 2, y0 + (2 - sy) * s + (s - m) / 2, m)

    corners = np.array([_square(500, 400, m), in_square(1, 2), in_square(2, 1), in_square(1, 0), in_square(0, 1)], np.float32)
    ids = np.array([50, 13, 12, 10, 11], np.int32)
    L = dr.layout(2.0)
    mg = dr.Margins()
    props = dr.proposals(L, 1.0, corners, mg)
    assert props == [None, None, None, (4, 2, 1), None]
    recs, _ = dr.detect(2.0, 1.0, ids, corners, 640, 480)
    assert len(recs) == 1
    r = recs[0]
    assert r["index"].tolist() == [3, 4, 2, 1] and r["ids"].tolist() == [10, 11, 12, 13]
    # the middle square's corners: top left, top right, bottom right, bottom left
    assert np.allclose(r["corners0"], [[180, 140], [260, 140], [260, 220], [180, 220]], rtol=0, atol=1e-3)
    assert r["win"].tolist() == [10, 10, 10, 10] and np.array_equal(r["corners"], r["corners0"])  # (20 sqrt 2 - 2 = 26 px, clamped; no image)
    assert dr.side(corners[0]) == 40.0
    # the right partners are matched exactly; the anchor's other candidates are whole squares away
    assert min(mg.tol) > 0.99 and min(mg.gap) > 1.0
    # with the tolerance below the noise nothing is matched; one partner moved by 0.9 of the tolerance is matched, by 1.1 not
    moved = corners.copy()
    moved[4] += np.float32([36.0, 0.0])
    assert len(dr.detect(2.0, 1.0, ids, moved, 640, 480)[0]) == 1
    moved[4] += np.float32([8.0, 0.0])
    assert len(dr.detect(2.0, 1.0, ids, moved, 640, 480)[0]) == 0
    # another corner order is another marker (checkAllOrders = false)
    turned = corners.copy()
    turned[2] = np.roll(turned[2], 1, axis=0)
    assert len(dr.detect(2.0, 1.0, ids, turned, 640, 480)[0]) == 0


def test_the_hand_made_cases_are_what_they_say():
    by = {c.name: c for c in dc.ALL}
    assert [len(by["one@%g" % r].want) for r in dc.ROLLS] == [1, 1, 1, 1]
    two = by["two shuffled"]
    assert [w["ids"].tolist() for w in two.want] == [[3, 3, 9, 3], [10, 11, 12, 13]] and [int(w["index"][0]) for w in two.want] == [9, 11]
    assert len(by["three of four"].want) == 0 and by["four equal ids"].want[0]["ids"].tolist() == [77] * 4
    assert len(by["corner in the margin"].want) == 0
    assert len(by["17 diamonds"].want) == 17 and len(by["17 diamonds"].ids) == 68
    assert len(by["64 diamonds"].want) == 64 and len(by["64 diamonds"].ids) == 256
    for c in dc.ALL:
        anchors = [int(w["index"][0]) for w in c.want]
        assert anchors == sorted(anchors)
        for w, truth in zip(c.want, c.truth or []):
            assert np.abs(w["corners0"] - truth).max() < 1.0  # (+-0.3 px of corner noise through two homographies)
        print(c.name, "markers", len(c.ids), "diamonds", len(c.want), "worst margin %.4g" % c.margins.worst())


def _check_rendered(fr, want_ids):
    """oracle.detect -> the restatement on a rendered frame: every diamond found with its ids, every refined corner within a quarter
    of the smallest projected square side of the truth.  A wrong partner is off by a whole square, so the bound is a condition, not a
    measurement."""
    import oracle
    ids, corners = oracle.detect(fr.image, dc.dictionary())
    recs, mg = dr.detect(dc.RATE, 1.0, ids, corners, dc.W, dc.H, gray=fr.image)
    assert sorted(r["ids"].tolist() for r in recs) == sorted(list(i) for i in want_ids)
    for r in recs:
        k = [list(i) for i in want_ids].index(r["ids"].tolist())
        truth = fr.corners_image[k]
        side = np.linalg.norm(truth - np.roll(truth, 1, axis=0), axis=1).min()
        e0, e1 = np.linalg.norm(r["corners0"] - truth, axis=1).max(), np.linalg.norm(r["corners"] - truth, axis=1).max()
        print("diamond", r["ids"].tolist(), "windows", r["win"].tolist(), "smallest square side %.1f px" % side,
              "interpolated: worst %.3f px, refined: worst %.3f px" % (e0, e1), "worst margin %.3g" % mg.worst())
        assert e0 < side / 4 and e1 < side / 4
        # the diamond as a fiducial of side square_len: its pose is the sheet's, at the middle square
        b, R, t = fr.diamonds[k]
        rv, tv, _ = oracle.solve_pnp_square(dc.K, dc.Z5, r["corners"], dc.SQUARE)
        assert np.abs(synth._rodrigues(rv) - R).max() < 0.03 and np.abs(tv - (R @ b.centre + t)).max() < 0.005  # (the fiducial's axes are the sheet's)
    return recs


def test_rendered_frontal_and_tilted_end_to_end_against_the_truth():
    _check_rendered(dc.frontal_frame(), [dc.ONE_IDS])
    _check_rendered(dc.one_frame(37.0), [dc.ONE_IDS])


def test_rendered_two_diamonds_and_loose_markers():
    recs = _check_rendered(dc.two_frame(), [ids for ids, *_ in dc.TWO])
    assert len(recs) == 2


# ---------------------------------------------------------------------------------------------------- the default of max_rep_rate
def measure_rep_rate(n_poses: int, seed: int):
    """Random poses of one diamond (tilt up to 0.6 rad about a random axis in the image plane, any roll, marker sides of about 12 to
    50 px), corner noise +-0.3 px, rate 0.04 / 0.024, the restatement's exact homography from the anchor -> per pose (side_a, the right
    partners' worst d / side_a, the closest wrong partner's d / side_a inside the diamond)."""
    rng = np.random.default_rng(seed)
    L = dr.layout(dc.RATE)
    obj = dc.diamond((0, 1, 2, 3)).marker_object_points.reshape(-1, 3)
    out = np.zeros((n_poses, 3))
    for p in range(n_poses):
        ang, phi = rng.uniform(0, 0.6), rng.uniform(0, 2 * np.pi)
        R, t = dc.diamond_pose((ang * np.cos(phi), ang * np.sin(phi), 0.0), dc.K[0, 0] * dc.MARKER / rng.uniform(12, 50), rng.uniform(0, 360),
                               (rng.uniform(-150, 150), rng.uniform(-100, 100)))
        c = (dc.project(obj, R, t, dc.K, dc.Z5).reshape(4, 4, 2) + rng.uniform(-dc.NOISE_PX, dc.NOISE_PX, (4, 4, 2))).astype(np.float32)
        h = dr.cr.homography4(L.marker_obj[0, :, :2], c[0].astype(np.float64))
        s = dr.side(c[0])
        right, wrong = 0.0, np.inf
        for k in (1, 2, 3):
            d = np.sqrt(dr._d2(dr._through(h, L.marker_obj[k]), c))
            right = max(right, d[k])
            wrong = min(wrong, min(d[j] for j in (1, 2, 3) if j != k))
        out[p] = (s, right / s, wrong / s)
    return out


def test_the_default_of_max_rep_rate_separates_right_from_wrong_partners():
    """The measurement recorded in fid_abi.h, repeated with a fixed seed: for markers of 30 px side and more the right partner stays
    below 1.0 marker sides and the closest wrong one above it."""
    m = measure_rep_rate(6000, 2024)
    s, right, wrong = m[:, 0], m[:, 1], m[:, 2]
    for lo, hi in ((30, 60), (20, 30), (0, 20)):
        sel = (s >= lo) & (s < hi)
        print("sides %d - %d px: %d poses, right partner d / side at most %.2f, closest wrong partner at least %.2f" % (lo, hi, sel.sum(), right[sel].max(), wrong[sel].min()))
    big = s >= 30
    assert big.sum() > 1000
    assert right[big].max() < dr.DEFAULT_MAX_REP_RATE < wrong[big].min()
    assert wrong.min() > 1.5  # (at every size: a wrong partner is most of a square away)
    assert right[s < 20].max() > 1.0  # (small markers do need a larger value)
