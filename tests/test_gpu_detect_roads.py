"""The roads of the detect launch sequence (fid_api.hip: enqueue_detect, its SubBatch views, Grids and stage functions), one case
per road at the smallest frame count that takes it.  Every case runs on a fresh detector created with the road's environment set
(and restored behind it), and every frame of every call must give the oracle's markers: the same ids and the same corners to the
last bit (np.array_equal on the float32 corners).  The calls of one, two and four frames are also checked stage by stage
(test_gpu_parity.check_stages).

Frames: the 333 x 275 and 384 x 272 frames of test_gpu_seedless_probe.py (four distinct ones, tiled to the call's frame count) with
two small synthetic markers (fiducials_amd/synth.py) pasted into their free corners, so that the candidate tail has quads to sort,
identify and refine.  The oracle runs once per distinct (frame, parameters) and is cached.

How a case knows that its road was taken -- only by what the library exposes already:
  * last_launches() (the sub-batches of the last call): the resident halves 64 / 36, FID_SUB_SHARES, FID_SUB_FRAMES, the four copy
    pieces of a host-fed call, FID_NO_FEED_OVERLAP (the host-fed call is then cut like a resident one);
  * FID_TAP_COUNTS slot 9 (nsurv1, written only by a first probe pass of two): calls of fewer than 16 frames take two passes, a call
    of 16 takes the single refilled pass;
  * FID_TAP_COUNTS slot 10 (nseeds): zero when the call was traced by the whole-border walk (FID_TRACE=legacy, and the rerun of a
    call whose seed tables overflowed), non-zero under cycle tracing.
Roads that cannot be recognised from outside (no hook is added for them; the cases still run them and check their results):
  * the index stream and FID_NO_IDX_STREAM, k_seg_cycles<48> and FID_NO_SEGC_WARM, the 256-workgroup walker cap (calls of one / two frames);
  * FID_STAGGER and FID_FS_BARRIER (event waits only), FID_FEED_SHARES (four pieces either way);
  * FID_PIECES=2 at 64 frames (two pieces, as the two halves are two sub-batches);
  * a chained submit (fid_order_after) at 16 frames (one sub-batch with or without the chain) and where FID_CHAIN_AT records tail_ev;
  * FID_SEED_KERNEL split / fused (the same starts and seeds either way);
  * which of the three threshold kernels ran, k_to_gray, k_refine_contour / k_subpix<7> / k_subpix<15>: their results are what the
    oracle comparison sees;
  * the context's `fallbacks` counter has no accessor: a fallback shows as nseeds == 0 on a context that traces by cycles."""
import functools
import os

import numpy as np
import pytest

import oracle
from fiducials_amd import _lib
from fiducials_amd.detector import ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary
from fiducials_amd.synth import make_frame
from helpers import n_scales
from test_gpu_parity import check_stages, params_pair
from test_gpu_seedless_probe import FrameOfBatch, seedless_frame

SIZES = [(333, 275), (384, 272)]
DICT = 6
PATCH_W, PATCH_H = 72, 78
PATCH_AT = ((258, 4), (256, 192))  # (x, y) of the two free corners of seedless_frame, clear of its shapes at every offset
ROAD_ENV = ("FID_NO_IDX_STREAM", "FID_NO_SEGC_WARM", "FID_SUB_SHARES", "FID_SUB_FRAMES", "FID_STAGGER", "FID_FS_BARRIER", "FID_PIECES",
            "FID_FEED_SHARES", "FID_NO_FEED_OVERLAP", "FID_CHAIN_AT", "FID_TRACE", "FID_SEED_KERNEL", "FID_SEED_SHIFT")
NODE, STEP8, WIDE = (), (("adaptiveThreshWinSizeMin", 5), ("adaptiveThreshWinSizeMax", 45), ("adaptiveThreshWinSizeStep", 8)), \
    (("adaptiveThreshWinSizeMin", 85), ("adaptiveThreshWinSizeMax", 93), ("adaptiveThreshWinSizeStep", 8))


@functools.lru_cache(maxsize=None)
def frames_of(size):
    """The four distinct frames of a size, read-only."""
    d = get_predefined_dictionary(DICT)
    out = []
    for k, variant in enumerate((0, 1, 4, 8)):
        img = seedless_frame(*size, variant)
        for j, (x, y) in enumerate(PATCH_AT):
            patch = make_frame(d, 500 + 10 * k + j, width=PATCH_W, height=PATCH_H, n_markers=1, side_range=(36.0, 44.0), max_tilt_deg=20.0)
            img[y:y + PATCH_H, x:x + PATCH_W] = patch.image
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


def batch_of(size, nframes):
    fr = frames_of(size)
    return np.ascontiguousarray(np.stack([fr[f % len(fr)] for f in range(nframes)]))


@functools.lru_cache(maxsize=None)
def want(size, k, table=()):
    """The oracle's (ids, corners) of distinct frame k under the parameter table: computed once, never changed."""
    _, op = params_pair(**dict(table))
    ids, corners = oracle.detect(frames_of(size)[k], get_predefined_dictionary(DICT), op)
    ids.setflags(write=False)
    corners.setflags(write=False)
    return ids, corners


def assert_oracle(results, size, table=()):
    for f, (corners, ids) in enumerate(results):
        oids, ocorners = want(size, f % 4, table)
        assert ids.tolist() == oids.tolist(), f
        assert corners.dtype == ocorners.dtype and np.array_equal(corners, ocorners), f


class road:
    """The environment of a road, set for the creation of the case's detectors and restored behind the case."""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        assert set(self.env) <= set(ROAD_ENV)
        self.saved = {k: os.environ.get(k) for k in ROAD_ENV}
        for k in ROAD_ENV:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def new_det(size, max_batch, table=(), **kw):
    p, _ = params_pair(**dict(table))
    return ArucoDetector(DICT, params=p, max_width=size[0], max_height=size[1], max_batch=max_batch, max_markers=32, **kw)


def counts(det, nframes):
    return det.tap_counts()[:nframes].copy()


def test_every_frame_has_markers_for_the_candidate_tail():
    """(no GPU) the oracle finds the pasted markers in every distinct frame, under every parameter table the cases use."""
    for size in SIZES:
        for k in range(4):
            assert len(want(size, k)[0]) >= 1
    for table in (STEP8, WIDE, (("cornerRefinementMethod", 2),), (("cornerRefinementWinSize", 9),)):
        assert sum(len(want(SIZES[0], k, table)[0]) for k in range(4)) >= 2


# ---- calls of a few frames: one piece, the index stream, two probe passes
FEW = [(1, {}), (2, {}), (4, {}), (1, {"FID_NO_IDX_STREAM": "1"}), (2, {"FID_NO_IDX_STREAM": "1"}), (1, {"FID_NO_SEGC_WARM": "1"}),
       (2, {"FID_NO_SEGC_WARM": "1"})]  # (the two switches act on the index stream and on k_seg_cycles<48>: calls of one or two frames)


@pytest.mark.gpu
@pytest.mark.parametrize("nframes,env", FEW, ids=["-".join([str(n)] + [k[4:].lower() for k in e]) for n, e in FEW])
@pytest.mark.parametrize("size", SIZES)
def test_calls_of_a_few_frames(size, nframes, env):
    d = get_predefined_dictionary(DICT)
    _, op = params_pair()
    with road(**env):
        det = new_det(size, nframes)
        try:
            batch = batch_of(size, nframes)
            if nframes == 1:
                check_stages(det, batch[0], d, op)
                results = [det.detect_markers(batch[0])]
            else:
                results = det.detect_markers_batch(batch)
                masks = det.tap_masks(nframes, n_scales(op), size[1], size[0])
                for f in range(nframes):
                    check_stages(FrameOfBatch(det, f, results, masks), batch[f], d, op)
            assert_oracle(results, size)
            cnt = counts(det, nframes)
            assert det.last_launches() == 1
            assert all(int(c[9]) >= int(c[7]) > 0 and int(c[10]) > 0 for c in cnt)  # two probe passes; seeds: cycle tracing
        finally:
            det.close()


# ---- a call of 16 frames: one piece, gm = 1, the single refilled probe pass
@pytest.mark.gpu
@pytest.mark.parametrize("seed_kernel", [None, "split", "fused"])
@pytest.mark.parametrize("nframes", [4, 16])
def test_seed_kernels_and_the_single_pass(nframes, seed_kernel):
    size = SIZES[nframes == 16]
    with road(**({"FID_SEED_KERNEL": seed_kernel} if seed_kernel else {})):
        det = new_det(size, nframes)
        try:
            assert_oracle(det.detect_markers_batch(batch_of(size, nframes)), size)
            cnt = counts(det, nframes)
            assert det.last_launches() == 1
            assert all(int(c[7]) > 0 and int(c[10]) > 0 for c in cnt)
            assert all((int(c[9]) == 0) == (nframes == 16) for c in cnt)  # (surv1 only behind a first pass of two)
        finally:
            det.close()


# ---- resident batches: sub-batches side by side, staggered, behind a barrier, as a chain of pieces
RESIDENT = [
    ("halves", 32, {}, 2),
    ("shares_50_30_20", 32, {"FID_SUB_SHARES": "50,30,20"}, 3),
    ("sub_frames_8", 32, {"FID_SUB_FRAMES": "8"}, 4),
    ("stagger", 32, {"FID_STAGGER": "1"}, 2),
    ("fs_barrier", 32, {"FID_FS_BARRIER": "1"}, 2),
    ("pieces_2", 64, {"FID_PIECES": "2"}, 2),
    ("legacy", 32, {"FID_TRACE": "legacy"}, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,nframes,env,nsub", RESIDENT, ids=[r[0] for r in RESIDENT])
def test_resident_batches(name, nframes, env, nsub):
    torch = pytest.importorskip("torch")
    size = SIZES[1]
    dev = torch.from_numpy(batch_of(size, nframes)).cuda()
    with road(**env):
        det = new_det(size, nframes)
        try:
            assert_oracle(det.detect_markers_device(dev.data_ptr(), nframes, size[0], size[1]), size)
            assert det.last_launches() == nsub
            cnt = counts(det, nframes)
            assert all((int(c[10]) == 0) == (name == "legacy") for c in cnt)  # (no seeds: the whole-border walk)
        finally:
            det.close()


@pytest.mark.gpu
def test_legacy_tracing_of_one_frame():
    size = SIZES[0]
    with road(FID_TRACE="legacy"):
        det = new_det(size, 1)
        try:
            check_stages(det, frames_of(size)[0], get_predefined_dictionary(DICT), params_pair()[1])
            cnt = counts(det, 1)
            assert det.last_launches() == 1 and int(cnt[0][10]) == 0 and int(cnt[0][7]) > 0
        finally:
            det.close()


# ---- frames from host memory: the copy's pieces
HOST_FED = [("pieces_20_30_30_20", {}, 4), ("feed_shares_25", {"FID_FEED_SHARES": "25,25,25,25"}, 4), ("no_feed_overlap", {"FID_NO_FEED_OVERLAP": "1"}, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,nsub", HOST_FED, ids=[r[0] for r in HOST_FED])
def test_host_fed_batches(name, env, nsub):
    size, nframes = SIZES[0], 64
    with road(**env):
        det = new_det(size, nframes)
        try:
            assert_oracle(det.detect_markers_batch(batch_of(size, nframes)), size)
            assert det.last_launches() == nsub
        finally:
            det.close()


# ---- batches in turn on two contexts (fid_order_after): where tail_ev is recorded
@pytest.mark.gpu
@pytest.mark.parametrize("chain_at", [0, 3, 5])
def test_two_contexts_in_turn(chain_at):
    torch = pytest.importorskip("torch")
    size, nframes = SIZES[1], 16
    dev = torch.from_numpy(batch_of(size, nframes)).cuda()
    with road(FID_CHAIN_AT=str(chain_at)):
        dets = [new_det(size, nframes) for _ in range(2)]
        try:
            dets[0].submit_device(dev.data_ptr(), nframes, size[0], size[1])
            for k in range(1, 5):  # (each submit ordered behind the batch in flight on the other context)
                dets[k & 1].submit_device(dev.data_ptr(), nframes, size[0], size[1], after=dets[(k - 1) & 1])
                assert_oracle(dets[(k - 1) & 1].collect(), size)
            assert_oracle(dets[0].collect(), size)
            assert all(d.last_launches() == 1 for d in dets)
        finally:
            for d in dets:
                d.close()


# ---- a call whose seed tables overflow is traced again by the whole-border walk
FALLBACK_CONTOURS = 1536  # (room for the ~900 probe survivors of a frame, not for its ~5400 seeds on the 32 px grid)


@pytest.mark.gpu
@pytest.mark.parametrize("nframes", [1, 4])
def test_forced_fallback_to_the_whole_border_walk(nframes):
    size = SIZES[0]
    with road(FID_SEED_SHIFT="2"):
        det = new_det(size, nframes, max_contours=FALLBACK_CONTOURS)
        try:
            for _ in range(2):  # (the fallback holds for one call: the next call tries its seeds again, and falls back again)
                assert_oracle(det.detect_markers_batch(batch_of(size, nframes)), size)
                cnt = counts(det, nframes)
                assert all(int(c[10]) == 0 and int(c[7]) > 0 and int(c[6]) == 0 for c in cnt)  # no seeds, survivors, no overflow left
        finally:
            det.close()
        roomy = new_det(size, nframes)  # (and with room for the seeds the same call traces by cycles)
        try:
            assert_oracle(roomy.detect_markers_batch(batch_of(size, nframes)), size)
            assert all(int(c[10]) > FALLBACK_CONTOURS for c in counts(roomy, nframes))
        finally:
            roomy.close()


# ---- the front: three threshold roads, colour input
@pytest.mark.gpu
@pytest.mark.parametrize("table", [NODE, STEP8, WIDE], ids=["node_table", "window_table", "wide_windows"])
@pytest.mark.parametrize("nframes", [1, 16])
def test_threshold_roads(nframes, table):
    size = SIZES[0]
    d = get_predefined_dictionary(DICT)
    with road():
        det = new_det(size, nframes, table)
        try:
            if nframes == 1:
                check_stages(det, frames_of(size)[0], d, params_pair(**dict(table))[1])
            else:
                assert_oracle(det.detect_markers_batch(batch_of(size, nframes)), size, table)
        finally:
            det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nframes", [1, 4])
def test_colour_input(nframes):
    size = SIZES[0]
    gray = batch_of(size, nframes).astype(np.int32)
    bgr = np.ascontiguousarray(np.stack([np.clip(gray + 12, 0, 255), gray, np.clip(gray - 9, 0, 255)], -1).astype(np.uint8))
    d = get_predefined_dictionary(DICT)
    with road():
        det = new_det(size, nframes)
        try:
            results = det.detect_markers_batch(bgr, encoding="bgr8")
            grays = det.tap(_lib.TAP_GRAY).reshape(nframes, size[1], size[0])
            for f in range(nframes):
                g = oracle.to_gray(bgr[f], _lib.ENC["bgr8"])
                assert np.array_equal(grays[f], g)
                oids, ocorners = oracle.detect(g, d)
                assert len(oids) >= 1 and results[f][1].tolist() == oids.tolist() and np.array_equal(results[f][0], ocorners)
        finally:
            det.close()


# ---- the end of the candidate tail: corner refinement by contour, by a sub-pixel window above 7
@pytest.mark.gpu
@pytest.mark.parametrize("table", [(("cornerRefinementMethod", 2),), (("cornerRefinementWinSize", 9),)], ids=["contour", "subpix_win_9"])
@pytest.mark.parametrize("nframes", [1, 16])
def test_corner_refinement_roads(nframes, table):
    size = SIZES[1]
    with road():
        det = new_det(size, nframes, table)
        try:
            results = det.detect_markers_batch(batch_of(size, nframes))
            assert_oracle(results, size, table)
            # (the road changes the corners: they are not the default parameters')
            assert any(len(r[1]) and not np.array_equal(r[0], want(size, f % 4)[1]) for f, r in enumerate(results))
        finally:
            det.close()
