"""One camera pose per frame from a map of fiducials on the device (k_map_pose, fid_set_map, fid_map_pose, fid_map_pose_last): the
kernel against the oracle's cv::solvePnP on hand-made markers, sets past the oracle's 32 points against an exact minimiser, end to
end on rendered boards and the recorded bag frame, batches and the submit / collect ring against the single-frame calls, and what
fid_set_map refuses.

The bound of the comparisons with the exact minimiser (numpy Gauss-Newton with the analytic Jacobian, started from the truth, run to a
step below 1e-14) is not chosen: CvLevMarq ends at 20 iterations / FLT_EPSILON, not at the minimum, so on the noisy coplanar cases of
<= 32 points the distance between the ORACLE and that minimiser is measured (aruco_map_cases.oracle_gap_to_minimum: 1.4e-9 when
this file was written) and ten times the largest such distance is allowed (FACTOR)."""
import functools

import numpy as np
import pytest

import aruco_map_cases as mc
from fiducials_amd import _lib, synth
from fiducials_amd.detector import MAP_ENTRY_DTYPE, ArucoDetector, FidError, map_entries
from helpers import gold_json, load_gray

pytestmark = pytest.mark.gpu

FACTOR = 10.0
Z5 = np.zeros(5)


@pytest.fixture(scope="module")
def det():
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=4, max_markers=32)
    yield d
    d.close()


def _dist(Ra, ta, Rb, tb) -> float:
    return float(max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max()))


def _check_record(got):
    """R is Rodrigues(rvec); cam_R, cam_t are the inverse of (R, tvec)."""
    assert np.abs(got["R"] - synth._rodrigues(got["rvec"])).max() < 1e-12
    assert np.abs(got["cam_R"] - got["R"].T).max() < 1e-12 and np.abs(got["cam_t"] + got["R"].T @ got["tvec"]).max() < 1e-12


def _mean_squared_error_with_the_oracle(P, img, rvec, tvec, Dv) -> float:
    """getReprojectionError over the points: ora_project_points (float object points, <= 64 of them), projections rounded to float."""
    import ctypes as C

    import oracle
    Pf = np.ascontiguousarray(P, np.float32)
    assert np.array_equal(Pf.astype(np.float64), P)  # (the boards of this check are exact in float)
    prj = np.zeros((len(P), 2))
    Kc, Dc = np.ascontiguousarray(mc.K).reshape(9), np.ascontiguousarray(Dv, dtype=np.float64)
    r, t = np.ascontiguousarray(rvec), np.ascontiguousarray(tvec)
    oracle.lib().ora_project_points.restype = C.c_int
    rc = oracle.lib().ora_project_points(Kc.ctypes.data_as(C.c_void_p), Dc.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                                         t.ctypes.data_as(C.c_void_p), Pf.ctypes.data_as(C.c_void_p), len(P), prj.ctypes.data_as(C.c_void_p))
    assert rc == 0
    d = img - prj.astype(np.float32).astype(np.float64)
    return float((d * d).sum() / len(P))


# ------------------------------------------------------------------------------------------------ the kernel, no image
def test_one_marker_with_an_identity_entry_is_fid_pose(det):
    """The same four coplanar points: rvec / tvec equal estimatePoseSingleMarkers' (k_pose) to 1e-6."""
    det.set_map(map_entries([3], 0.14, [np.eye(3)], [np.zeros(3)]))
    rng = np.random.default_rng(5)
    for Dv in (Z5, mc.D_NONZERO):
        for _ in range(4):
            Rc, tc = mc.seeded_pose(rng)
            R = Rc @ mc.FACING
            c = mc.split_markers(mc.project(mc.fid_corners(0.14), R, tc, mc.K, Dv) + rng.uniform(-mc.NOISE_PX, mc.NOISE_PX, (4, 2)))
            got = det.map_pose(mc.K, Dv, c, [3])
            one = det.estimate_pose_single_markers(c, [3], 0.14, mc.K, Dv)
            assert got["n_markers"] == 1 and got["n_over"] == 0
            assert np.abs(got["rvec"] - one.rvecs[0]).max() < 1e-6 and np.abs(got["tvec"] - one.tvecs[0]).max() < 1e-6
            _check_record(got)
    det.set_map(None)


def test_coplanar_boards_match_the_oracle(det):
    """Boards of 2, 5 and 8 markers (8, 20, 32 points) in the planes z, x, y = const of the map and an oblique one of 5, exact and
    +-0.3 px noisy projections, with and without distortion: R and tvec to 1e-6 against cv::solvePnP restated on the same points in
    the same order; exact projections give the pose back."""
    import oracle
    worst = 0.0
    for name, Dv, R, t, P, exact, noisy in mc.planar_cases():
        e = mc.planar_board(name)
        det.set_map(e)
        for img in (exact, noisy):
            got = det.map_pose(mc.K, Dv, mc.split_markers(img), e["id"])
            assert got["n_markers"] == len(e) and got["n_over"] == 0
            r, tv = oracle.solve_pnp_points(mc.K, Dv, P, img)
            d = _dist(got["R"], got["tvec"], synth._rodrigues(r), tv)
            worst = max(worst, d)
            print("coplanar", name, "distance to the oracle", d)
            assert d < 1e-6, (name, Dv.tolist(), d)
            _check_record(got)
            if name != "oblique5":
                want = _mean_squared_error_with_the_oracle(P, img, got["rvec"], got["tvec"], Dv)
            else:  # (its corners are not exact in float: the same sum with the projection in double)
                dd = img - mc.project(P, got["R"], got["tvec"], mc.K, Dv).astype(np.float32).astype(np.float64)
                want = float((dd * dd).sum() / len(P))
            assert abs(got["image_error"] - want) < 1e-9, (name, got["image_error"], want)
        got = det.map_pose(mc.K, Dv, mc.split_markers(exact), e["id"])
        assert _dist(got["R"], got["tvec"], R, t) < 1e-6
    print("coplanar parity: largest distance to the oracle", worst)
    det.set_map(None)


@pytest.mark.parametrize("n_a,n_b", [(3, 3), (1, 1)])
def test_non_coplanar_sets(det, n_a, n_b):
    """Two walls at right angles.  Exact projections give the pose back to 1e-6.  The oracle has no non-planar branch (it answers -4
    for these sets), so the noisy comparison with it is dropped; instead the noisy result is held to the exact minimiser of the same
    reprojection error within FACTOR x the oracle's own gap."""
    import oracle
    e = mc.corner_of_two_walls(n_a, n_b)
    P = mc.object_points(e)
    det.set_map(e)
    bound = FACTOR * mc.oracle_gap_to_minimum()
    rng = np.random.default_rng(100 * n_a + n_b)
    for Dv in (Z5, mc.D_NONZERO):
        for _ in range(3):
            eye = np.array([0.2, 0.0, 0.2]) + rng.uniform(0.7, 1.1) * synth._rodrigues(rng.uniform(-0.25, 0.25, 3)) @ np.array([0.7, 0.1, 0.7])
            R, t = mc.look_at(eye, [0.2, 0.0, 0.2])
            exact = mc.project(P, R, t, mc.K, Dv).astype(np.float32).astype(np.float64)
            got = det.map_pose(mc.K, Dv, mc.split_markers(exact), e["id"])
            assert got["n_markers"] == n_a + n_b
            d = _dist(got["R"], got["tvec"], R, t)
            assert d < 1e-6, (n_a, n_b, d)
            noisy = (exact + rng.uniform(-mc.NOISE_PX, mc.NOISE_PX, exact.shape)).astype(np.float32).astype(np.float64)
            with pytest.raises(AssertionError):
                oracle.solve_pnp_points(mc.K, Dv, P, noisy)  # (the day it takes them, compare with it to 1e-6 here)
            got = det.map_pose(mc.K, Dv, mc.split_markers(noisy), e["id"])
            Rm, tm = mc.exact_minimiser(P, noisy, R, t, mc.K, Dv)
            d = _dist(got["R"], got["tvec"], Rm, tm)
            print("non-coplanar", n_a, n_b, "noisy: distance to the exact minimum", d, "bound", bound)
            assert d < bound, (n_a, n_b, d, bound)
            _check_record(got)
    det.set_map(None)


@functools.lru_cache(maxsize=None)
def _large_case(n_markers: int, noisy: bool):
    """An oblique board of n_markers on a 16-wide grid, seen from far enough: (entries, P, R, t, image points as floats)."""
    Rb, tb = mc.OBLIQUE, np.array([0.05, -0.02, 0.3])
    e = mc.grid_board(n_markers, 16, Rb, tb, first_id=100)
    P = mc.object_points(e)
    rng = np.random.default_rng(n_markers)
    R, t = mc.board_pose(rng, Rb, tb, tz_range=(3.0, 4.0))
    img = mc.project(P, R, t, mc.K, mc.D_NONZERO * 0.2)
    if noisy:
        img = img + rng.uniform(-mc.NOISE_PX, mc.NOISE_PX, img.shape)
    return e, P, R, t, img.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n_markers", [17, 64, 256, 257])
def test_sizes_only_this_kernel_meets(det, n_markers):
    """17 markers (68 points: the first stride wrap), 64, 256 (the LDS cap) and 257 (one over: n_markers 256, n_over 1)."""
    Dv = mc.D_NONZERO * 0.2
    used = min(n_markers, _lib.MAP_MAX_USED)
    bound = FACTOR * mc.oracle_gap_to_minimum()
    e, P, R, t, exact = _large_case(n_markers, False)
    det.set_map(e)
    got = det.map_pose(mc.K, Dv, mc.split_markers(exact), e["id"])
    assert got["n_markers"] == used and got["n_over"] == n_markers - used
    d = _dist(got["R"], got["tvec"], R, t)
    print(n_markers, "markers, exact projections: distance to the pose", d)
    assert d < 1e-6, (n_markers, d)
    _, _, _, _, noisy = _large_case(n_markers, True)
    got = det.map_pose(mc.K, Dv, mc.split_markers(noisy), e["id"])
    assert got["n_markers"] == used and got["n_over"] == n_markers - used
    Rm, tm = mc.exact_minimiser(P[:4 * used], noisy[:4 * used], R, t, mc.K, Dv)
    d = _dist(got["R"], got["tvec"], Rm, tm)
    print(n_markers, "markers, noisy: distance to the exact minimum", d, "bound", bound)
    assert d < bound, (n_markers, d, bound)
    dd = noisy[:4 * used] - mc.project(P[:4 * used], got["R"], got["tvec"], mc.K, Dv).astype(np.float32).astype(np.float64)
    assert abs(got["image_error"] - float((dd * dd).sum() / (4 * used))) < 1e-9
    _check_record(got)
    assert det.map_pose(mc.K, Dv, mc.split_markers(noisy), e["id"]).tobytes() == got.tobytes()  # reproducible bit for bit
    det.set_map(None)


def test_bookkeeping_of_the_marker_list(det):
    import oracle
    name, Dv, R, t, P, exact, noisy = [c for c in mc.planar_cases() if c[0] == "floor8" and c[1].any()][0]
    e = mc.planar_board(name)
    det.set_map(e)
    bound = FACTOR * mc.oracle_gap_to_minimum()
    c = mc.split_markers(noisy)
    ids = e["id"].copy()
    base = det.map_pose(mc.K, Dv, c, ids)
    # another list order: the same pose within the stop rule's slack (the points enter the sums in another order)
    order = [5, 0, 7, 2, 1, 6, 3, 4]
    got = det.map_pose(mc.K, Dv, c[order], ids[order])
    assert got["n_markers"] == 8 and _dist(got["R"], got["tvec"], base["R"], base["tvec"]) < bound
    r, tv = oracle.solve_pnp_points(mc.K, Dv, P.reshape(8, 4, 3)[order].reshape(-1, 3), noisy.reshape(8, 4, 2)[order].reshape(-1, 2))
    assert _dist(got["R"], got["tvec"], synth._rodrigues(r), tv) < 1e-6
    # ids the map does not name are passed over, wherever they stand
    stray = (c[:1] + 33.0, [900])
    got = det.map_pose(mc.K, Dv, np.concatenate([stray[0], c[:3], stray[0] + 5.0, c[3:]]), np.concatenate([stray[1], ids[:3], [-7], ids[3:]]))
    assert got["n_markers"] == 8 and got.tobytes() == base.tobytes()
    # an id that stands twice in the list is left out altogether: the pose of the list without it
    without = det.map_pose(mc.K, Dv, np.delete(c, 2, axis=0), np.delete(ids, 2))
    twice = det.map_pose(mc.K, Dv, np.concatenate([c, c[2:3] + 50.0]), np.concatenate([ids, ids[2:3]]))
    assert without["n_markers"] == 7 and twice.tobytes() == without.tobytes() and twice["n_over"] == 0
    # nothing of the map in the list: no pose, zeros
    none = det.map_pose(mc.K, Dv, stray[0], stray[1])
    assert none["n_markers"] == 0 and none.tobytes() == np.zeros(1, none.dtype).tobytes()
    assert det.map_pose(mc.K, Dv, np.zeros((0, 4, 2)), []).tobytes() == none.tobytes()
    det.set_map(None)


def test_a_full_map_with_the_used_ids_at_both_ends(det):
    """4 096 entries; the markers in sight are the first and the last entries of the sorted table (and the map is handed over unsorted)."""
    name, Dv, R, t, P, exact, noisy = [c for c in mc.planar_cases() if c[0] == "flat2" and c[1].any()][0]
    two = mc.planar_board(name)
    det.set_map(two)
    want = det.map_pose(mc.K, Dv, mc.split_markers(noisy), two["id"])
    full = np.zeros(_lib.MAP_MAX_ENTRIES, MAP_ENTRY_DTYPE)
    full["id"] = 5000 + 3 * np.arange(len(full))
    full["len"] = 0.1
    full["R"] = np.eye(3)
    full["t"] = np.stack([np.arange(len(full)) * 0.5, np.ones(len(full)), np.zeros(len(full))], axis=1)
    full[[0, -1]] = two
    full["id"][0], full["id"][-1] = -2_000_000_000, 2_000_000_000
    rng = np.random.default_rng(1)
    det.set_map(full[rng.permutation(len(full))])
    got = det.map_pose(mc.K, Dv, mc.split_markers(noisy), [-2_000_000_000, 2_000_000_000])
    assert got["n_markers"] == 2 and got.tobytes() == want.tobytes()
    det.set_map(None)


def test_set_map_refusals(det):
    L = _lib.load()

    def rc(entries):
        e = np.ascontiguousarray(entries, dtype=MAP_ENTRY_DTYPE)
        return L.fid_set_map(det._ctx, e.ctypes.data, len(e))

    good = mc.scene_map("2x2")
    fr = mc.scene("2x2", 0)
    det.set_map(good)
    det.detect_markers(fr.image)
    before = det.map_pose_last(mc.K, None)
    assert before["n_markers"].tolist() == [4]
    many = np.zeros(_lib.MAP_MAX_ENTRIES + 1, MAP_ENTRY_DTYPE)
    many["id"], many["len"], many["R"] = np.arange(len(many)), 0.1, np.eye(3)
    assert rc(many) == _lib.FID_E_UNSUPPORTED and b"4096" in L.fid_last_error(det._ctx)
    assert rc(many[:-1]) == _lib.FID_OK
    det.set_map(good)
    for bad_len in (0.0, -0.1, np.nan):
        bad = good.copy()
        bad["len"][1] = bad_len
        assert rc(bad) == _lib.FID_E_INVALID_ARG and b"len" in L.fid_last_error(det._ctx)
    twice = good.copy()
    twice["id"][3] = twice["id"][0]
    assert rc(twice) == _lib.FID_E_INVALID_ARG
    # a refused map leaves the one before it in place
    det.detect_markers(fr.image)
    assert det.map_pose_last(mc.K, None).tobytes() == before.tobytes()
    # n = 0 clears it: fid_map_pose_last and fid_map_pose refuse
    det.set_map(None)
    for call in (lambda: det.map_pose_last(mc.K, None), lambda: det.map_pose(mc.K, None, fr.corners_image, fr.ids)):
        with pytest.raises(FidError) as ex:
            call()
        assert ex.value.status == _lib.FID_E_INVALID_ARG


# ------------------------------------------------------------------------------------------------ end to end
def _oracle_or_minimiser(entries, ids, corners, Dv, R0, t0, Kc=mc.K):
    """The reference pose for detected corners: the oracle's solvePnP where it takes the set (coplanar); for the two-wall corner,
    which it refuses, the exact minimiser next to the rendering pose stands in for it -- a stricter reference than the oracle, which
    itself stops within oracle_gap_to_minimum() of that minimiser -- under the same 1e-6."""
    import oracle
    P = mc.map_points_for(entries, ids)
    img = np.asarray(corners, np.float64).reshape(-1, 2)
    try:
        r, tv = oracle.solve_pnp_points(Kc, Dv, P, img)
        return synth._rodrigues(r), tv, 1e-6
    except AssertionError:
        Rm, tm = mc.exact_minimiser(P, img, R0, t0, Kc, Dv)
        return Rm, tm, 1e-6


@pytest.mark.parametrize("name,pose", mc.SCENES)
def test_end_to_end_on_rendered_scenes(det, name, pose):
    fr = mc.scene(name, pose)
    e = mc.scene_map(name)
    det.set_map(e)
    corners, ids = det.detect_markers(fr.image)
    assert sorted(ids.tolist()) == fr.ids.tolist()
    last = det.map_pose_last(mc.K, None)
    assert len(last) == 1 and last[0]["n_markers"] == len(ids)
    assert last[0].tobytes() == det.map_pose(mc.K, None, corners, ids).tobytes()
    # ... and once the camera is known, the detect call itself has run the kernel: the same record again
    corners2, ids2 = det.detect_markers(fr.image)
    assert np.array_equal(corners2, corners) and det.map_pose_last(mc.K, None).tobytes() == last.tobytes()
    Rw, tw, bound = _oracle_or_minimiser(e, ids, corners, Z5, fr.R, fr.tvec)
    d = _dist(last[0]["R"], last[0]["tvec"], Rw, tw)
    assert d < bound, (name, pose, d, bound)
    _check_record(last[0])
    print(name, pose, "distance to the rendering pose: R", np.abs(last[0]["R"] - fr.R).max(), "t", np.abs(last[0]["tvec"] - fr.tvec).max(),
          "image_error", last[0]["image_error"])
    det.set_map(None)


def test_an_occluded_marker_leaves_a_pose_from_the_rest(det):
    e = mc.scene_map("3x2")
    fr = mc.scene("3x2", 1, without=2)
    det.set_map(e)
    corners, ids = det.detect_markers(fr.image)
    assert sorted(ids.tolist()) == [20, 21, 23, 24, 25]
    got = det.map_pose_last(mc.K, None)[0]
    Rw, tw, bound = _oracle_or_minimiser(e, ids, corners, Z5, fr.R, fr.tvec)
    assert got["n_markers"] == 5 and _dist(got["R"], got["tvec"], Rw, tw) < bound
    assert np.linalg.norm(got["tvec"] - fr.tvec) < 0.02 * np.linalg.norm(fr.tvec)
    det.set_map(None)


def test_the_recorded_bag_frame_puts_the_camera_at_the_map_origin():
    """aruco_images.bag seq 4957, 7 markers: a map whose T_map_fid are the recorded per-marker transforms has the camera at its
    origin.  The joint pose over the 28 points is held to 1e-6.  The seven recorded transforms do not lie in one plane (each is its own
    noisy four-point pose), so the oracle's solvePnP, which has no non-planar branch, answers -4 for this set; the exact minimiser next
    to the identity stands in for it (_oracle_or_minimiser)."""
    b = gold_json()["bag_4957"]
    rec = b["transforms"]["transforms"]
    Rs = []
    for t in rec:
        x, y, z, w = t["rotation_xyzw"]
        Rs.append(np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]))
    e = map_entries([t["fiducial_id"] for t in rec], 0.14, Rs, [t["translation"] for t in rec])
    gray = load_gray("bag_4957")
    det7 = ArucoDetector(7, max_width=gray.shape[1], max_height=gray.shape[0])
    try:
        det7.set_map(e)
        corners, ids = det7.detect_markers(gray)
        assert ids.tolist() == [t["fiducial_id"] for t in rec]
        got = det7.map_pose_last(b["K"], b["D"])[0]
        assert got["n_markers"] == 7
        Rw, tw, bound = _oracle_or_minimiser(e, ids, corners, np.asarray(b["D"], float)[:5], np.eye(3), np.zeros(3), np.asarray(b["K"], float).reshape(3, 3))
        d = _dist(got["R"], got["tvec"], Rw, tw)
        print("bag frame: distance to the reference pose", d, "; from the identity: R", np.abs(got["R"] - np.eye(3)).max(), "t", np.abs(got["tvec"]).max(),
              "image_error", got["image_error"])
        assert d < bound, d
        _check_record(got)
    finally:
        det7.close()


@functools.lru_cache(maxsize=None)
def _batch_frames():
    """0, 1, 4 and 6 mapped markers with the 3 x 2 board's map, the empty frame first: the 2 x 2 board's scene (none of its ids is in
    the map), then one, four and all six markers of the 3 x 2 board."""
    e = mc.scene_map("3x2")
    d = mc.get_predefined_dictionary(mc.DICT)

    def some(keep, pose, seed):
        return synth.make_aruco_board_frame(d, e["id"][keep], [(float(e["len"][k]), e["R"][k], e["t"][k]) for k in keep], mc.K, *mc.scene_pose("3x2", pose),
                                            seed, mc.W, mc.H)

    one, four = some([4], 0, 9), some([1, 2, 4, 5], 2, 10)
    frames = np.stack([mc.scene("2x2", 1).image, one.image, four.image, mc.scene("3x2", 1).image])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _single_frame_results():
    d = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=4, max_markers=32)
    try:
        d.set_map(mc.scene_map("3x2"))
        out = []
        for img in _batch_frames():
            corners, ids = d.detect_markers(img)
            out.append((corners, ids, d.pose_last(mc.SCENE_LEN, mc.K, mc.D_NONZERO)[0], d.map_pose_last(mc.K, mc.D_NONZERO)[0].copy(), d.last_launches()))
        return out
    finally:
        d.close()


def test_a_batch_equals_the_single_frame_calls(det):
    want = _single_frame_results()
    assert [int(w[3]["n_markers"]) for w in want] == [0, 1, 4, 6] and len(want[0][1]) == 4
    det.set_map(mc.scene_map("3x2"))
    for round_ in range(2):  # the second round: the camera is known, the detect call runs the kernel in its own stream
        res = det.detect_markers_batch(_batch_frames())
        mp = det.map_pose_last(mc.K, mc.D_NONZERO)
        assert len(mp) == 4
        for f in range(4):
            assert np.array_equal(res[f][0], want[f][0]) and np.array_equal(res[f][1], want[f][1])
            assert mp[f].tobytes() == want[f][3].tobytes(), (round_, f)
    det.set_map(None)


def test_the_submit_collect_ring_on_two_contexts():
    want = _single_frame_results()
    frames = np.ascontiguousarray(_batch_frames())
    dets = [ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=4, max_markers=32) for _ in range(2)]
    try:
        for d in dets:
            d.set_map(mc.scene_map("3x2"))
        dets[0].submit_batch(frames)
        for k in range(1, 5):
            dets[k % 2].submit_batch(frames, after=dets[(k - 1) % 2])
            d = dets[(k - 1) % 2]
            res = d.collect()
            with pytest.raises(FidError):
                dets[k % 2].map_pose_last(mc.K, mc.D_NONZERO)  # a batch is in flight there
            mp = d.map_pose_last(mc.K, mc.D_NONZERO)
            for f in range(4):
                assert np.array_equal(res[f][0], want[f][0]) and mp[f].tobytes() == want[f][3].tobytes(), (k, f)
        dets[0].collect()
    finally:
        for d in dets:
            d.close()


def test_a_map_changes_nothing_else(det):
    """Markers and fid_pose_last byte-identical with and without a map; fid_last_launches with a map at most one more than without,
    and the parent's count again once the map is cleared."""
    frames = _batch_frames()

    def run():
        res = det.detect_markers_batch(frames)
        poses = det.pose_last(mc.SCENE_LEN, mc.K, mc.D_NONZERO)
        res = det.detect_markers_batch(frames)  # (the camera known: the pose kernels ride in the detect call)
        poses2 = det.pose_last(mc.SCENE_LEN, mc.K, mc.D_NONZERO)
        blob = b"".join(r[0].tobytes() + r[1].tobytes() for r in res) + b"".join(p.rvecs.tobytes() + p.tvecs.tobytes() + p.image_error.tobytes() for p in poses2)
        assert blob[-1:] and all(np.array_equal(a.rvecs, b.rvecs) for a, b in zip(poses, poses2))
        return blob, det.last_launches()

    det.set_map(None)
    plain, launches_plain = run()
    det.set_map(mc.scene_map("3x2"))
    det.detect_markers_batch(frames)
    det.map_pose_last(mc.K, mc.D_NONZERO)
    mapped, launches_mapped = run()
    assert det.map_pose_last(mc.K, mc.D_NONZERO)["n_markers"].tolist() == [0, 1, 4, 6]
    det.set_map(None)
    cleared, launches_cleared = run()
    assert mapped == plain == cleared
    assert launches_plain <= launches_mapped <= launches_plain + 1 and launches_cleared == launches_plain
