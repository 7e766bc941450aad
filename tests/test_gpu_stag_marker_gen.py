"""The markers fiducials_amd.stag_marker_gen draws, through the device detector: the frames of
tests/test_stag_marker_gen.py (every HD library, ids 0, 1, the last and 5 at random, 3 sizes x 4 rotations x 2 tilts) read
frame by frame from host memory and from a torch tensor, and as one batch with a pose per marker."""
import numpy as np
import pytest
import torch

from fiducials_amd import stag as fstag
from fiducials_amd import stag_marker_gen as smg
from oracle import stag_ref
from test_stag_marker_gen import MARKER_SIZE, view_frames

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hd", smg.HD_VALUES)
def test_generated_markers_on_the_device(hd):
    """Each frame read by StagDetector.detect_markers, by detect_markers_device from a torch tensor and by
    StagPool.detect_markers_batch with K / D / marker_size: the same markers on all three roads, and the reference's own
    Stag::detectMarkers' (oracle/_ref) ids with corners and centre within the refined path's 1e-3 px; where oracle/_ref is not
    built, the generated id (at most one view of an id read as nothing, as the reference reads these frames) with corners
    within 2 px of the projected square.  The pose of each marker, printed at side_mm = 1000 * marker_size: the recovered
    tvec within 1 % of the true one (measured: up to 0.97 % at 72 px across = 3.5 m, 0.44 % at 110 px, 0.34 % at 170 px)."""
    ec = (hd - 1) // 2
    cases = view_frames(hd)
    size = cases[0][2].shape[0]
    live = stag_ref.available()
    det = fstag.StagDetector(hd, ec, max_width=size, max_height=size)
    pool = fstag.StagPool(hd, ec, n_contexts=4, max_width=size, max_height=size)
    try:
        single, missed = [], {}
        for mid, view, img, corners, _, _ in cases:
            M = det.detect_markers(img)
            t = torch.from_numpy(img).to("cuda")
            torch.cuda.synchronize()
            Md = det.detect_markers_device(t.data_ptr(), size, size)
            assert np.array_equal(Md, M), (mid, view)
            if live:
                ref = stag_ref.detect_markers(img, hd, ec)
                assert M["id"].tolist() == ref[:, 0].astype(int).tolist(), (mid, view, M["id"], ref[:, 0])
                if len(M):
                    assert np.abs(M["corners"].reshape(-1, 8) - ref[:, 1:9]).max() < 1e-3, (mid, view)
                    assert np.abs(M["center"] - ref[:, 9:11]).max() < 1e-3, (mid, view)
            assert M["id"].tolist() in ([mid], []), (mid, view, M["id"])
            if len(M):
                assert np.linalg.norm(M["corners"][0] - corners, axis=1).max() < 2.0, (mid, view)
            else:
                missed[mid] = missed.get(mid, 0) + 1
            single.append(M)
        assert max(missed.values(), default=0) <= 1, missed
        K = cases[0][5]
        ms, ps = pool.detect_markers_batch(np.stack([c[2] for c in cases]), K, None, MARKER_SIZE)
        worst = {}
        for (mid, view, _, _, tvec, _), M, m, p in zip(cases, single, ms, ps):
            assert np.array_equal(m["id"], M["id"]) and np.array_equal(m["corners"], M["corners"]), (mid, view)
            if len(p):
                assert p["id"][0] == mid
                err = np.linalg.norm(p["tvec"][0] - tvec) / np.linalg.norm(tvec)
                worst[view[0]] = max(worst.get(view[0], 0.0), err)
        print("HD%d: views read as nothing %s, worst tvec error by size %s" % (hd, missed, {k: round(v, 4) for k, v in worst.items()}))
        assert max(worst.values()) < 0.01, worst
    finally:
        det.close()
        pool.close()
