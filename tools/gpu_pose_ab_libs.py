#!/usr/bin/env python3
"""Two builds of the library on the same inputs of the solvePnP kernels (k_pose, k_stag_pose, k_stag_bundle_pose, k_map_pose plain and
with its covariance, k_map_pose_robust, k_charuco_pose; csrc/fid_pnp.h): every pose record the library returns must be the same
BYTES -- the library is built with -ffp-contract=off and without fast-math, so a change that keeps every operand and every order
keeps every bit, and a mismatch names a place where an order changed.  The inputs are small and all come from the case modules
under tests/:
  k_pose              every case of the 14 pose_cases.PAIRS, one call per pair with a length per marker (as test_gpu_pose_sweep.pose);
                      one call of 65 markers (a partial ninth wave)
  k_stag_pose         pose_cases.stag_frames() (1, 3, 4, 5, 9 markers) x 14 pairs x STAG_SIZES through pose_last; the group form on
                      the 64-slot batch below
  k_stag_bundle_pose  test_gpu_stag_bundles.planar_cases() (1, 2, 4, 6 tags; exact and noisy; with and without distortion) through
                      bundle_pose; the two non-coplanar sets of 6 and 12 tags; one batch of 64 slots (the group form)
  k_map_pose          aruco_map_cases.planar_cases() (2, 5, 8 markers and the oblique board of 5) through map_pose; the non-coplanar
                      sets (3, 3) and (1, 1); 17, 64, 256 and 257 markers; a list with a duplicated id; a batch of 4
  k_map_pose_cov      the same lists and the same batch through map_pose_cov / map_pose_cov_last: pose and covariance records
  k_map_pose_robust   every case of map_robust_cases.cases() -- the bookkeeping list, the re-admission and the four-solves case (several
                      solves over subsets with holes), the equidistant frame with a marker past 89 degrees among them --; a batch of
                      four frames with four outcomes: pose and robust records
  k_charuco_pose      through charuco_pose: 4 corners not on one line, the few and collinear records, a distorted view under each
                      camera model, an equidistant view with a corner beyond the model (void), a rendered view with a hidden marker,
                      63, 64, 65 and 72 corners of the 10 x 9 board, the 462 corners of the 22 x 23 board
Usage: gpu_pose_ab_libs.py <libA.so> <libB.so>      two children, one after the other: never two processes with the GPU open
       AB_CHILD=1 FID_LIB=<lib.so> gpu_pose_ab_libs.py      one build: a JSON line {kernel: [[sha256 of a call's records, records], ...]}
                                                            (the program to put behind `rocprofv3 --kernel-trace --stats --`)"""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
KERNELS = ("k_pose", "k_stag_pose", "k_stag_bundle_pose", "k_map_pose", "k_map_pose_cov", "k_map_pose_robust", "k_charuco_pose")
CHILD_TIMEOUT_S = 420


def child():
    import numpy as np
    import aruco_map_cases as mc
    import camera_model_cases as cm
    import charuco_cases as cc
    import map_robust_cases as rc
    import pose_cases as pc
    import stag_bundle_cases as bc
    import test_gpu_aruco_map as tm
    import test_gpu_map_robust as tr
    import test_gpu_stag_bundles as tb
    from fiducials_amd import stag as fstag, synth
    from fiducials_amd.camera import Camera
    from fiducials_amd.detector import ArucoDetector
    from fiducials_amd.dictionary import get_predefined_dictionary

    out = {k: [] for k in KERNELS}

    def put(kernel, blob: bytes, n: int):
        out[kernel].append([hashlib.sha256(blob).hexdigest()[:16], int(n)])

    # ---- k_pose
    det = ArucoDetector(get_predefined_dictionary("DICT_4X4_50"), max_width=640, max_height=480)

    def pose(corners, lengths, K, D):
        distinct = sorted(set(float(v) for v in lengths))
        ids = np.array([distinct.index(float(v)) for v in lengths], dtype=np.int32)
        pr = det.estimate_pose_single_markers(np.asarray(corners, np.float32).reshape(-1, 4, 2), ids, 0.14, K, D, {i: v for i, v in enumerate(distinct)})
        rec = np.ascontiguousarray(np.column_stack([pr.rvecs, pr.tvecs, pr.image_error, pr.object_error, pr.fiducial_area]), dtype=np.float64)
        put("k_pose", rec.tobytes(), len(rec))

    for cam, dist in pc.PAIRS:
        cs = pc.cases_for(cam, dist)
        pose(np.stack([c.corners for c in cs]), [c.length for c in cs], pc.camera_matrix(cam), pc.dist_coeffs(dist))
    cs = pc.cases_for("hd", "mild")[:65]
    pose(np.stack([c.corners for c in cs]), [c.length for c in cs], pc.camera_matrix("hd"), pc.dist_coeffs("mild"))
    det.close()

    # ---- k_stag_pose
    sdet = fstag.StagDetector(21, 7, max_width=pc.STAG_FRAME_SIZE[0], max_height=pc.STAG_FRAME_SIZE[1])
    for n_markers, img in pc.stag_frames():
        assert len(sdet.detect_markers(img)) == n_markers
        for cam, dist in pc.PAIRS:
            for size in pc.STAG_SIZES:
                P = sdet.pose_last(pc.camera_matrix(cam), pc.dist_coeffs(dist), size)
                put("k_stag_pose", P.tobytes(), len(P))
    sdet.close()

    # ---- k_stag_bundle_pose
    bdet = fstag.StagDetector(21, 7, max_width=bc.W, max_height=bc.H)

    def bundle(Dv, ids, img):
        got = bdet.bundle_pose(bc.K, Dv, bc.markers_from_points(ids, img.reshape(len(ids), 5, 2)))
        put("k_stag_bundle_pose", got.tobytes(), len(got))

    bdet.set_layout(fstag.board_layout(range(6), bc.oblique_board(6)))
    for n, Dv, R, t, P, exact, noisy in tb.planar_cases():
        for img in (exact, noisy):
            bundle(Dv, range(n), img)
    for n_tags in (6, 12):  # (test_non_coplanar_sets' poses)
        corners = bc.two_faces(n_tags)
        P = bc.tags_points(corners)
        bdet.set_layout(fstag.board_layout(range(n_tags), corners))
        rng = np.random.default_rng(77 + n_tags)
        for Dv in (np.zeros(5), bc.D_NONZERO):
            for _ in range(6):
                R0, t = bc.seeded_pose(rng, tilt_deg=(0.0, 15.0))
                exact = bc.project(P, R0 @ synth._rodrigues(np.array([0.0, -np.pi / 4, 0.0])), t, bc.K, Dv)
                bundle(Dv, range(n_tags), exact)
                bundle(Dv, range(n_tags), exact + rng.uniform(-tb.NOISE_PX, tb.NOISE_PX, size=exact.shape))
    bdet.close()
    pool = fstag.StagPool(21, 7, n_contexts=64, max_width=bc.W, max_height=bc.H)
    pool.set_layout(tb._scene_layout("hd21_3x2"))
    M, P, B = pool.detect_bundles_batch(np.concatenate([tb._batch_frames()] * 8), bc.K, bc.D_NONZERO, 0.08)
    for f in range(len(M)):
        put("k_stag_pose", P[f].tobytes(), len(P[f]))
        put("k_stag_bundle_pose", B[f].tobytes(), len(B[f]))
    pool.close()

    # ---- k_map_pose and k_map_pose_cov: the same lists through fid_map_pose_cam and fid_map_pose_cov_cam
    mdet = ArucoDetector(mc.DICT, max_width=mc.W, max_height=mc.H, max_batch=4, max_markers=32)

    def map_pose(Dv, img, ids):
        corners = mc.split_markers(img) if img.ndim == 2 else img
        put("k_map_pose", mdet.map_pose(mc.K, Dv, corners, ids).tobytes(), 1)
        got, cov = mdet.map_pose_cov(mc.K, Dv, corners, ids, sigma_px=1.0)
        put("k_map_pose_cov", got.tobytes() + cov.tobytes(), 1)

    for name, Dv, R, t, P, exact, noisy in mc.planar_cases():
        e = mc.planar_board(name)
        mdet.set_map(e)
        for img in (exact, noisy):
            map_pose(Dv, img, e["id"])
        if name == "floor8" and Dv.any():  # (test_bookkeeping_of_the_marker_list's list with an id that stands twice)
            c = mc.split_markers(noisy)
            map_pose(Dv, np.concatenate([c, c[2:3] + 50.0]), np.concatenate([e["id"], e["id"][2:3]]))
    for n_a, n_b in ((3, 3), (1, 1)):  # (test_non_coplanar_sets' views)
        e = mc.corner_of_two_walls(n_a, n_b)
        P = mc.object_points(e)
        mdet.set_map(e)
        rng = np.random.default_rng(100 * n_a + n_b)
        for Dv in (np.zeros(5), mc.D_NONZERO):
            for _ in range(3):
                eye = np.array([0.2, 0.0, 0.2]) + rng.uniform(0.7, 1.1) * synth._rodrigues(rng.uniform(-0.25, 0.25, 3)) @ np.array([0.7, 0.1, 0.7])
                R, t = mc.look_at(eye, [0.2, 0.0, 0.2])
                exact = mc.project(P, R, t, mc.K, Dv).astype(np.float32).astype(np.float64)
                map_pose(Dv, exact, e["id"])
                map_pose(Dv, (exact + rng.uniform(-mc.NOISE_PX, mc.NOISE_PX, exact.shape)).astype(np.float32).astype(np.float64), e["id"])
    for n_markers in (17, 64, 256, 257):
        for noisy in (False, True):
            e, P, R, t, img = tm._large_case(n_markers, noisy)
            mdet.set_map(e)
            map_pose(mc.D_NONZERO * 0.2, img, e["id"])
    mdet.set_map(mc.scene_map("3x2"))
    mdet.detect_markers_batch(tm._batch_frames())
    mp = mdet.map_pose_last(mc.K, mc.D_NONZERO)
    put("k_map_pose", mp.tobytes(), len(mp))
    mp, mcov = mdet.map_pose_cov_last(mc.K, mc.D_NONZERO, sigma_px=1.0)
    put("k_map_pose_cov", mp.tobytes() + mcov.tobytes(), len(mp))

    # ---- k_map_pose_robust: every planted case (the bookkeeping list, the re-admission and four-solves cases, whose subsets have
    # holes, and the equidistant frame with a marker past 89 degrees are among them), then a batch of four outcomes
    for c in rc.cases().values():
        mdet.set_map(c.entries)
        pose, rob = mdet.map_pose_robust(camera=Camera(c.model, mc.K, c.D), corners=c.corners, ids=c.ids, inlier_px=c.inlier_px, min_markers=c.min_markers)
        put("k_map_pose_robust", pose.tobytes() + rob.tobytes(), 1)
    mdet.set_map(tr._lying_map())
    mdet.detect_markers_batch(tr._batch_frames())
    poses, robs = mdet.map_pose_robust_last(camera=tr.CAM_D, inlier_px=rc.INLIER_PX, min_markers=2)
    put("k_map_pose_robust", poses.tobytes() + robs.tobytes(), len(poses))
    mdet.close()

    # ---- k_charuco_pose, through fid_charuco_pose_cam
    cdet = ArucoDetector(cc.DICT, max_width=cc.W, max_height=cc.H, max_markers=256)
    Z5 = np.zeros(5)

    def corner_view(bname, ids, tilt, dist, roll, seed, model=cm.PLUMB_BOB, D=Z5):
        """the board's corners `ids` seen from a pose under a camera model, +-0.3 px of seeded noise, as float32"""
        R, t = cc.board_pose(bname, tilt, dist, roll)
        xy = cm.project(model, cc.K, D, R, t, cc.rboard(bname).corner_obj[ids])
        return (xy + np.random.default_rng(seed).uniform(-cc.NOISE_PX, cc.NOISE_PX, xy.shape)).astype(np.float32)

    def charuco_pose(xy, ids, model=cm.PLUMB_BOB, D=Z5):
        put("k_charuco_pose", cdet.charuco_pose(xy, ids, camera=Camera(model, cc.K, D)).tobytes(), 1)

    cdet.set_charuco_board(cc.board("5x4"))
    for ids in ([0, 1, 2, 7], [0, 5, 10], [], [0, 1, 2, 3], [1, 5, 9, 9]):  # four corners not on one line; few; one line
        charuco_pose(corner_view("5x4", ids, (0.2, -0.1, 0.0), 0.36, 0.1, 40), ids)
    all12 = list(range(12))
    for model, D in ((cm.PLUMB_BOB, cc.D_NONZERO * 4), cm.SETS["prism12"], cm.SETS["fe_kb"]):  # a distorted view under each model
        charuco_pose(corner_view("5x4", all12, (0.45, -0.3, 0.0), 0.40, 0.25, 41, model, D), all12, model, D)
    beyond = corner_view("5x4", all12, (0.1, 0.2, 0.0), 0.46, -0.4, 42, cm.EQUIDISTANT, (0.0,) * 4)
    beyond[3, 0] = cc.K[0, 2] + 2.0 * cc.K[0, 0]  # theta_d = 2 rad: past 89 degrees, the record is void
    charuco_pose(beyond, all12, cm.EQUIDISTANT, (0.0,) * 4)
    cdet.detect_markers(cc.view("tilted", hidden=(3,)).image)  # a rendered view with a hidden marker: the refined corners it gives
    rec = cdet.charuco_last(K=cc.K, D=Z5)[0]
    charuco_pose(np.stack([rec["x"], rec["y"]], axis=1), rec["id"])
    cdet.set_charuco_board(cc.board("10x9"))
    for n in (63, 64, 65, 72):  # the first stride, its end, the second stride, the whole board
        charuco_pose(corner_view("10x9", list(range(n)), (0.2, -0.15, 0.0), 0.36, 0.1, 43 + n, D=cc.D_NONZERO), list(range(n)), D=cc.D_NONZERO)
    cdet.set_charuco_board(cc.board("22x23"))  # the largest board: 462 corners
    charuco_pose(corner_view("22x23", list(range(462)), (0.05, -0.05, 0.0), 0.74, 0.0, 44), list(range(462)))
    cdet.close()
    print(json.dumps(out))


def main():
    if os.environ.get("AB_CHILD") == "1":
        child()
        return 0
    res = []
    for lib in sys.argv[1:3]:
        try:  # (a child that hangs is killed at its own limit and no other is started)
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, AB_CHILD="1", FID_LIB=os.path.abspath(lib)), capture_output=True,
                               text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print("no result from", lib, "within", CHILD_TIMEOUT_S, "s")
            return 2
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode or not lines:
            print("no result from", lib, "exit", p.returncode, p.stderr[-800:])
            return 2
        res.append(json.loads(lines[-1]))
    a, b = res
    parts, bad = [], 0
    for k in KERNELS:
        wrong = [i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y] + list(range(min(len(a[k]), len(b[k])), max(len(a[k]), len(b[k]))))
        bad += len(wrong)
        parts.append(f"{k} {sum(n for _, n in a[k])} records in {len(a[k])} calls, mismatching calls {len(wrong)} {wrong[:6] if wrong else ''}".rstrip())
    print("pose A/B of two builds: " + "; ".join(parts) + f"; mismatches {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
