"""Tag bundles on the device (k_stag_bundle_pose, fid_stag_bundle_pose*, fid_stag_detect_bundles_batch*): the kernel against the
oracle's cv::solvePnP on hand-made markers, non-coplanar sets against an exact minimiser, end to end on rendered boards, the batch
roads against the single-frame calls, and what fid_stag_set_layout refuses."""
import functools

import numpy as np
import pytest

import stag_bundle_cases as bc
from fiducials_amd import _lib, stag as fstag, synth

pytestmark = pytest.mark.gpu

NOISE_PX = 0.3


@pytest.fixture(scope="module")
def det():
    d = fstag.StagDetector(21, 7, max_width=bc.W, max_height=bc.H)
    yield d
    d.close()


def _dist(Ra, ta, Rb, tb) -> float:
    return float(max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max()))


@functools.lru_cache(maxsize=None)
def planar_cases():
    """Test 1's cases, made once: (n_tags, D, R, t, object points, image points exact, image points noisy)."""
    out = []
    rng = np.random.default_rng(2024)
    for n in (1, 2, 4, 6):
        P = bc.tags_points(bc.oblique_board(6)[:n])
        for Dv in (np.zeros(5), bc.D_NONZERO):
            for _ in range(6):
                R, t = bc.seeded_pose(rng)
                img = bc.project(P, R, t, bc.K, Dv)
                out.append((n, Dv, R, t, P, img, img + rng.uniform(-NOISE_PX, NOISE_PX, size=img.shape)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_gap_to_minimum() -> float:
    """The largest distance between oracle.solve_pnp_points and the exact minimiser of the same reprojection error over the noisy
    planar cases: what the oracle's 20-iteration / FLT_EPSILON stop leaves."""
    import oracle
    worst = 0.0
    for n, Dv, R, t, P, _, noisy in planar_cases():
        r, tv = oracle.solve_pnp_points(bc.K, Dv, P, noisy)
        Rm, tm = bc.exact_minimiser(P, noisy, R, t, bc.K, Dv)
        worst = max(worst, _dist(synth._rodrigues(r), tv, Rm, tm))
    return worst


def test_planar_kernel_matches_the_oracle_without_a_frame(det):
    """bundle_pose on hand-made markers: 5 ... 30 coplanar points in an oblique plane of the bundle frame, with and without
    distortion, exact and noisy projections: R and tvec to 1e-6 against cv::solvePnP restated on the same points in the same order."""
    import oracle
    det.set_layout(fstag.board_layout(range(6), bc.oblique_board(6)))
    worst = 0.0
    for n, Dv, R, t, P, exact, noisy in planar_cases():
        for img in (exact, noisy):
            m = bc.markers_from_points(range(n), img.reshape(n, 5, 2))
            got = det.bundle_pose(bc.K, Dv, m)
            assert len(got) == 1 and got["bundle"][0] == 0 and got["n_tags"][0] == n
            r, tv = oracle.solve_pnp_points(bc.K, Dv, P, img)
            d = _dist(got["R"][0], got["tvec"][0], synth._rodrigues(r), tv)
            worst = max(worst, d)
            assert d < 1e-6, (n, Dv.tolist(), d, got["rvec"][0], r)
            assert np.abs(got["R"][0] - synth._rodrigues(got["rvec"][0])).max() < 1e-12
        # the exact projections give the pose back
        got = det.bundle_pose(bc.K, Dv, bc.markers_from_points(range(n), exact.reshape(n, 5, 2)))
        assert _dist(got["R"][0], got["tvec"][0], R, t) < 1e-6
    print("planar parity: largest distance to the oracle", worst)
    det.set_layout(None)


def test_markers_in_another_order_and_unknown_ids(det):
    """The points go in marker order (solvePnpBundle walks the marker list); ids the layout does not name are passed over; a run is
    reproducible bit for bit."""
    import oracle
    corners = bc.oblique_board(6)
    det.set_layout(fstag.board_layout(range(6), corners))
    n, Dv, R, t, P, exact, noisy = planar_cases()[-1]
    order = [4, 0, 5, 2]
    img5 = noisy.reshape(6, 5, 2)[order]
    m = bc.markers_from_points(order, img5)
    stray = bc.markers_from_points([77], img5[:1] + 40.0)
    mixed = np.concatenate([m[:2], stray, m[2:]])
    got = det.bundle_pose(bc.K, Dv, mixed)
    assert got["n_tags"].tolist() == [4]
    r, tv = oracle.solve_pnp_points(bc.K, Dv, bc.tags_points(corners[order]), img5.reshape(-1, 2))
    assert _dist(got["R"][0], got["tvec"][0], synth._rodrigues(r), tv) < 1e-6
    assert det.bundle_pose(bc.K, Dv, mixed).tobytes() == got.tobytes()
    assert len(det.bundle_pose(bc.K, Dv, stray)) == 0
    det.set_layout(None)


@pytest.mark.parametrize("n_tags", [6, 12])
def test_non_coplanar_sets(det, n_tags):
    """Tags on two faces at 90 degrees: 30 points, and 60 (past the oracle's 32).  The oracle refuses them (no non-planar branch), so
    (a) exact projections must give the pose back to 1e-6, (b) with +-0.3 px noise the result is compared with an exact minimiser of
    the same reprojection error; the bound is 10 x what the ORACLE leaves to that minimiser on the noisy planar cases (its stop rule:
    20 iterations / FLT_EPSILON), the factor for the other conditioning of a two-plane set."""
    corners = bc.two_faces(n_tags)
    P = bc.tags_points(corners)
    det.set_layout(fstag.board_layout(range(n_tags), corners))
    bound = 10.0 * oracle_gap_to_minimum()
    rng = np.random.default_rng(77 + n_tags)
    worst_exact = worst_noisy = 0.0
    for Dv in (np.zeros(5), bc.D_NONZERO):
        for _ in range(6):
            R0, t = bc.seeded_pose(rng, tilt_deg=(0.0, 15.0))
            R = R0 @ synth._rodrigues(np.array([0.0, -np.pi / 4, 0.0]))  # both faces at about 45 degrees to the view
            exact = bc.project(P, R, t, bc.K, Dv)
            got = det.bundle_pose(bc.K, Dv, bc.markers_from_points(range(n_tags), exact.reshape(n_tags, 5, 2)))
            assert got["n_tags"].tolist() == [n_tags]
            d = _dist(got["R"][0], got["tvec"][0], R, t)
            worst_exact = max(worst_exact, d)
            assert d < 1e-6, (n_tags, d)
            noisy = exact + rng.uniform(-NOISE_PX, NOISE_PX, size=exact.shape)
            got = det.bundle_pose(bc.K, Dv, bc.markers_from_points(range(n_tags), noisy.reshape(n_tags, 5, 2)))
            Rm, tm = bc.exact_minimiser(P, noisy, R, t, bc.K, Dv)
            d = _dist(got["R"][0], got["tvec"][0], Rm, tm)
            worst_noisy = max(worst_noisy, d)
            print("non-coplanar", n_tags, "noisy: distance to the exact minimum", d, "bound", bound)
            assert d < bound, (n_tags, d, bound)
            assert np.abs(got["R"][0] - synth._rodrigues(got["rvec"][0])).max() < 1e-12
    print("non-coplanar", n_tags, "worst exact", worst_exact, "worst noisy", worst_noisy, "oracle gap", oracle_gap_to_minimum())
    det.set_layout(None)


def _paint_over(image, quad, value=235):
    """The image with the quad (4, 2), grown by a fifth about its centre, filled."""
    c = quad.mean(axis=0)
    q = c + (quad - c) * 1.2
    yy, xx = np.mgrid[0:image.shape[0], 0:image.shape[1]]
    inside = np.ones(image.shape, bool)
    for i in range(4):
        a, b = q[i], q[(i + 1) % 4]
        inside &= (b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0]) >= 0
    out = image.copy()
    out[inside] = value
    return out


@functools.lru_cache(maxsize=None)
def occluded(pose: int):
    fr = bc.scene("hd21_2x2", pose)
    img = fr.image
    for k in (1, 2):
        img = _paint_over(img, fr.corners_image[k])
    img.setflags(write=False)
    return img


def _scene_layout(board):
    fr = bc.scene(board, 0)
    return fstag.board_layout(fr.ids, fr.corners_board)


@pytest.mark.parametrize("board,pose", bc.hd21_scenes())
def test_end_to_end_on_the_board_scenes(det, board, pose):
    import oracle
    fr = bc.scene(board, pose)
    det.set_layout(_scene_layout(board))
    M = det.detect_markers(fr.image)
    assert sorted(M["id"].tolist()) == list(fr.ids)
    last = det.bundle_pose_last(bc.K, None)
    assert last.tobytes() == det.bundle_pose(bc.K, None, M).tobytes()
    assert last["bundle"].tolist() == [0] and last["n_tags"].tolist() == [len(fr.ids)]
    r, t = oracle.solve_pnp_points(bc.K, np.zeros(5), bc.board_points(fr, M["id"]), bc.marker_points(M))
    assert _dist(last["R"][0], last["tvec"][0], synth._rodrigues(r), t) < 1e-6
    assert np.linalg.norm(last["tvec"][0] - fr.tvec) < 0.02 * np.linalg.norm(fr.tvec)
    assert bc.angle_deg(last["R"][0][:, 2], fr.R[:, 2]) < 1.0
    det.set_layout(None)


def test_occluded_tags_and_bundles_out_of_sight(det):
    import oracle
    fr = bc.scene("hd21_2x2", 1)
    # a second bundle none of whose tags is in the picture
    other = fstag.board_layout([10, 11], bc.oblique_board(2))
    lay = _scene_layout("hd21_2x2")
    tags = np.concatenate([other.tags, lay.tags])
    tags["bundle"][len(other.tags):] = 1
    det.set_layout(fstag.Layout(tags, ["elsewhere", "board"], np.zeros(2, bool)))
    M = det.detect_markers(occluded(1))
    assert sorted(M["id"].tolist()) == [0, 3]
    got = det.bundle_pose_last(bc.K, None)
    assert got["bundle"].tolist() == [1] and got["n_tags"].tolist() == [2]
    r, t = oracle.solve_pnp_points(bc.K, np.zeros(5), bc.board_points(fr, M["id"]), bc.marker_points(M))
    assert _dist(got["R"][0], got["tvec"][0], synth._rodrigues(r), t) < 1e-6
    assert np.linalg.norm(got["tvec"][0] - fr.tvec) < 0.02 * np.linalg.norm(fr.tvec)
    # nothing of any bundle in sight: no record
    flat = np.full((bc.H, bc.W), 150, np.uint8)
    assert len(det.detect_markers(flat)) == 0 and len(det.bundle_pose_last(bc.K, None)) == 0
    det.set_layout(None)


def test_standalone_tags_of_two_sizes_in_one_frame(det):
    """Two loose tags, 0.08 m and 0.05 m, each posed from its own corners; and fid_stag_pose_last does not care about the layout."""
    import oracle
    Ra, ta = bc.pose_of(0.3, 0.45)
    Rb, tb = bc.pose_of(-0.25, 0.40)
    ta, tb = ta + np.array([-0.09, 0.0, 0.0]), tb + np.array([0.10, 0.02, 0.0])
    A = synth.make_stag_board_frame(21, [4], 1, 1, bc.K, Ra, ta, 11, bc.W, bc.H, 96, 0.08, 40, noise_sigma=0.0)
    B = synth.make_stag_board_frame(21, [9], 1, 1, bc.K, Rb, tb, 12, bc.W, bc.H, 96, 0.05, 40, noise_sigma=0.0)
    img = np.where(B.image != 150, B.image, A.image).astype(np.float32)
    img = np.clip(np.rint(img + np.random.default_rng(13).normal(0, 2.0, img.shape)), 0, 255).astype(np.uint8)
    tags = np.concatenate([fstag.board_layout([4], A.corners_board).tags, fstag.board_layout([9], B.corners_board).tags])
    tags["bundle"] = [0, 1]
    det.set_layout(fstag.Layout(tags, ["tag_4", "tag_9"], np.ones(2, bool)))
    M = det.detect_markers(img)
    assert sorted(M["id"].tolist()) == [4, 9]
    got = det.bundle_pose_last(bc.K, bc.D_NONZERO)
    assert got["bundle"].tolist() == [0, 1] and got["n_tags"].tolist() == [1, 1]
    for k, fr in enumerate((A, B)):
        mk = M[M["id"] == fr.ids[0]]
        r, t = oracle.solve_pnp_points(bc.K, bc.D_NONZERO, bc.board_points(fr, fr.ids), bc.marker_points(mk))
        assert _dist(got["R"][k], got["tvec"][k], synth._rodrigues(r), t) < 1e-6
    got0 = det.bundle_pose_last(bc.K, None)
    for k, fr in enumerate((A, B)):
        assert np.linalg.norm(got0["tvec"][k] - fr.tvec) < 0.02 * np.linalg.norm(fr.tvec)
    with_layout = det.pose_last(bc.K, None, 0.08)
    det.set_layout(None)
    plain = fstag.StagDetector(21, 7, max_width=bc.W, max_height=bc.H)
    try:
        assert plain.detect_markers(img).tobytes() == M.tobytes()
        assert plain.pose_last(bc.K, None, 0.08).tobytes() == with_layout.tobytes()
        assert len(plain.bundle_pose_last(bc.K, None)) == 0  # no layout: no records
    finally:
        plain.close()


def _batch_frames():
    return np.stack([bc.scene(b, p).image for b, p in bc.hd21_scenes()] + [occluded(0), occluded(2)])


@functools.lru_cache(maxsize=None)
def _single_frame_results():
    """The eight frames one by one on one context with the 3 x 2 board's layout: (markers, bundle poses) per frame."""
    d = fstag.StagDetector(21, 7, max_width=bc.W, max_height=bc.H)
    try:
        d.set_layout(_scene_layout("hd21_3x2"))
        out = []
        for img in _batch_frames():
            M = d.detect_markers(img)
            out.append((M, d.bundle_pose_last(bc.K, bc.D_NONZERO)))
        return out
    finally:
        d.close()


def _check_batch(pool, frames, want):
    torch = pytest.importorskip("torch")
    F = len(frames)
    M0, P0 = pool.detect_markers_batch(frames, bc.K, bc.D_NONZERO, 0.08)
    M1, P1, B1 = pool.detect_bundles_batch(frames, bc.K, bc.D_NONZERO, 0.08)
    t = torch.from_numpy(np.ascontiguousarray(frames)).to("cuda")
    torch.cuda.synchronize()
    M2, P2, B2 = pool.detect_bundles_batch_device(t.data_ptr(), F, bc.W, bc.H, bc.K, bc.D_NONZERO, marker_size=0.08)
    for f in range(F):
        wm, wb = want[f % len(want)]
        assert len(wb) == 1
        for M, P, B in ((M1, P1, B1), (M2, P2, B2)):
            assert M[f].tobytes() == M0[f].tobytes() == wm.tobytes(), f
            assert P[f].tobytes() == P0[f].tobytes(), f
            assert B[f].tobytes() == wb.tobytes(), f


def test_batch_of_four_slots_equals_the_single_frame_calls():
    want = _single_frame_results()
    assert [int(b["n_tags"][0]) for _, b in want] == [4, 4, 4, 6, 6, 6, 2, 2]
    pool = fstag.StagPool(21, 7, n_contexts=4, max_width=bc.W, max_height=bc.H)
    try:
        pool.set_layout(_scene_layout("hd21_3x2"))
        _check_batch(pool, _batch_frames(), want)
        # contexts with different layouts, or with none, are refused
        pool.dets[2].set_layout(_scene_layout("hd21_2x2"))
        with pytest.raises(fstag.FidError) as e:
            pool.detect_bundles_batch(_batch_frames(), bc.K, None, 0.08)
        assert e.value.status == _lib.FID_E_INVALID_ARG
        pool.set_layout(None)
        with pytest.raises(fstag.FidError):
            pool.detect_bundles_batch(_batch_frames(), bc.K, None, 0.08)
        M, P = pool.detect_markers_batch(_batch_frames(), bc.K, bc.D_NONZERO, 0.08)  # ... and the plain call goes on as before
        assert M[3].tobytes() == want[3][0].tobytes()
    finally:
        pool.close()


def test_batch_of_64_slots_runs_the_group_form_of_the_kernel():
    """64 slots: groups of 32 frames, the kernel behind the trampoline with the frames as a grid dimension."""
    want = _single_frame_results()
    pool = fstag.StagPool(21, 7, n_contexts=64, max_width=bc.W, max_height=bc.H)
    try:
        pool.set_layout(_scene_layout("hd21_3x2"))
        _check_batch(pool, np.concatenate([_batch_frames()] * 8), want)
    finally:
        pool.close()


def test_set_layout_refusals(det):
    L = _lib.load()

    def rc(tags, n_bundles, d=det):
        t = np.ascontiguousarray(tags, dtype=fstag.TAG_DTYPE)
        return L.fid_stag_set_layout(d._ctx, t.ctypes.data, len(t), n_bundles)

    good = _scene_layout("hd21_2x2")
    det.set_layout(good)
    M = det.detect_markers(bc.scene("hd21_2x2", 0).image)
    before = det.bundle_pose_last(bc.K, None)
    assert len(before) == 1
    square = bc.oblique_board(1)[0]
    twice = good.tags.copy()
    twice["id"][1] = twice["id"][0]
    assert rc(twice, 1) == _lib.FID_E_INVALID_ARG  # an id listed twice
    outside = good.tags.copy()
    outside["id"][0] = len(fstag.load_library(21)) // 4
    assert rc(outside, 1) == _lib.FID_E_INVALID_ARG  # an id outside the library
    outside["id"][0] = -1
    assert rc(outside, 1) == _lib.FID_E_INVALID_ARG
    equal = good.tags.copy()
    equal["corners"][2, 1] = equal["corners"][2, 0]
    assert rc(equal, 1) == _lib.FID_E_INVALID_ARG  # a tag with two equal corners
    # the two size bounds, on a library with enough ids (HD21 has 12, HD11 thousands)
    det11 = fstag.StagDetector(11, 2, max_width=64, max_height=64)
    try:
        many = np.array([fstag.tag_from_three_corners(i, i, *square[:3]) for i in range(65)], dtype=fstag.TAG_DTYPE)
        assert rc(many, 65, det11) == _lib.FID_E_UNSUPPORTED  # more than 64 bundles
        assert rc(many[:64], 64, det11) == _lib.FID_OK
        crowd = np.array([fstag.tag_from_three_corners(i, 0, *square[:3]) for i in range(13)], dtype=fstag.TAG_DTYPE)
        assert rc(crowd, 1, det11) == _lib.FID_E_UNSUPPORTED  # more than 12 tags in a bundle
        assert rc(crowd[:12], 1, det11) == _lib.FID_OK
    finally:
        det11.close()
    hole = good.tags.copy()
    hole["bundle"] = [0, 0, 2, 2]
    assert rc(hole, 3) == _lib.FID_E_INVALID_ARG  # an empty bundle
    # a refused layout leaves the one before it in place
    det.set_layout(good)
    assert rc(twice, 1) == _lib.FID_E_INVALID_ARG
    assert det.bundle_pose_last(bc.K, None).tobytes() == before.tobytes()
    # n_tags = 0 clears it: no records
    det.set_layout(None)
    assert len(det.bundle_pose_last(bc.K, None)) == 0 and len(det.bundle_pose(bc.K, None, M)) == 0
