"""The reference of the ChArUco calibration tests on its own (no GPU): the keep rule for every case of charuco_calib_cases, the
selection rules of include/fid_abi.h ("camera calibration from ChArUco corners") on hand-written views, and the restatement
recovering the generating camera from noise-free views."""
import numpy as np
import pytest

import calib_cases as cc
import charuco_calib_cases as ccc
import charuco_calib_restatement as ccr


@pytest.mark.parametrize("model_name,shape", ccc.CASES + [ccc.CHUNK])
def test_every_case_passes_the_keep_rule(model_name, shape):
    ref = ccc.reference(model_name, shape)
    print(f"{model_name} {shape}: cost auto {ref['auto']['cost']:.6e} given {ref['given']['cost']:.6e} gap {ref['gap']:.2e} "
          f"std_dev gap {ref['gap_std']:.2e} rms gap {ref['gap_rms']:.2e} iterations {ref['auto']['iterations']} / {ref['given']['iterations']}")
    assert ref["gap"] <= cc.KEEP_GAP
    assert ref["stood_still"], "the reference was still moving at calib_restatement.lm's iteration cap"
    assert ref["kept"]
    c = ccc.case(model_name, shape)
    assert ref["best"]["used"] == list(range(len(c["views"])))
    assert ref["best"]["n_points"] == sum(len(i) for i, _ in c["views"])


def test_the_disturbed_case_keeps_and_uses_the_views_it_should():
    ref = ccc.disturbed_reference()
    assert ref["kept"], ref["gap"]
    best = ref["best"]
    assert best["statuses"] == [ccr.VIEW_FEW, ccr.VIEW_USED, ccr.VIEW_NO_START, ccr.VIEW_USED, ccr.VIEW_USED, ccr.VIEW_FEW]
    assert best["n_used"] == [3, 72, 9, 71, 72, 7]
    assert best["used"] == [1, 3, 4] and best["n_points"] == 72 + 71 + 72
    five = ccc.row_of_five_reference()
    assert five["kept"], five["gap"]
    assert five["best"]["statuses"] == [ccr.VIEW_USED, ccr.VIEW_NO_START, ccr.VIEW_USED] and five["best"]["n_used"] == [72, 5, 72]


def test_selection_on_hand_written_views():
    b = ccc.rboard("5x4")  # a 4 x 3 grid of corners, id = 4 cy + cx
    xy = lambda n: np.arange(2 * n, dtype=np.float32).reshape(n, 2)
    # list order is kept; an id listed twice is left out altogether
    ids = [5, 2, 9, 2, 0, 11]
    assert ccr.select(b, (ids, xy(6))) == [0, 2, 4, 5]
    obj, img, used = ccr.view_points(b, (ids, xy(6)))
    assert list(used) == [5, 9, 0, 11]
    assert (obj == b.corner_obj[[5, 9, 0, 11]]).all() and (img == xy(6)[[0, 2, 4, 5]]).all()
    # the object point of id i: ((cx + 1) s, (cy + 1) s, 0), each coordinate rounded through float
    s = 0.04
    assert (b.corner_obj[9] == np.array([2 * s, 3 * s, 0.0]).astype(np.float32).astype(np.float64)).all()
    # record arrays as charuco_last returns them: x0, y0 and win are ignored
    rec = np.zeros(3, [("id", "<i4"), ("win", "<i4"), ("x", "<f4"), ("y", "<f4"), ("x0", "<f4"), ("y0", "<f4")])
    rec["id"], rec["x"], rec["y"], rec["x0"], rec["win"] = [3, 4, 8], [1.5, 2.5, 3.5], [7.0, 8.0, 9.0], np.nan, 99
    obj, img, used = ccr.view_points(b, rec)
    assert list(used) == [3, 4, 8] and (img == [[1.5, 7.0], [2.5, 8.0], [3.5, 9.0]]).all()
    # fewer than max(min_points, 4) used points: FEW -- counted after the duplicates are out
    assert ccr.view_status(b, ([0, 1, 5], xy(3))) == ccr.VIEW_FEW
    assert ccr.view_status(b, ([0, 1, 5, 6, 6, 6], xy(6))) == ccr.VIEW_FEW
    assert ccr.view_status(b, ([0, 1, 5, 6], xy(4)), min_points=1) == ccr.VIEW_USED
    assert ccr.view_status(b, ([0, 1, 5, 6], xy(4)), min_points=5) == ccr.VIEW_FEW
    # on one line of the grid, tested exactly: a row, a column, a diagonal, a knight's line
    assert ccr.view_status(b, ([4, 5, 6, 7], xy(4))) == ccr.VIEW_NO_START
    assert ccr.view_status(b, ([1, 5, 9, 5, 1], xy(5)), min_points=1) == ccr.VIEW_FEW  # (one point is left)
    b10 = ccc.rboard("10x9")  # a 9 x 8 grid
    assert ccr.view_status(b10, ([0, 10, 20, 30, 40], xy(5))) == ccr.VIEW_NO_START
    assert ccr.view_status(b10, ([0, 11, 22, 33], xy(4))) == ccr.VIEW_NO_START  # (1, 2) steps: ids 0, 11 = (2, 1) ...
    assert ccr.view_status(b10, ([0, 11, 22, 34], xy(4))) == ccr.VIEW_USED
    # the refusals
    with pytest.raises(ValueError):
        ccr.select(b, ([0, 1, 12, 3], xy(4)))
    with pytest.raises(ValueError):
        ccr.select(b, ([0, 1, -1, 3], xy(4)))
    bad = xy(4)
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        ccr.select(b, ([0, 1, 2, 3], bad))


@pytest.mark.parametrize("model_name", list(ccc.MODELS))
def test_noise_free_views_give_the_generating_camera_back(model_name):
    """5 views x 462 corners without noise: what is left is the float32 rounding of the positions (at most 2^-14 px at 1 280), so the
    minimiser lies within a small multiple of its own std_dev of the generating values and the rms is of that size."""
    c, ref = ccc.case(model_name, "5x462_exact"), ccc.reference(model_name, "5x462_exact")
    best = ref["best"]
    free = [i for i in range(16) if c["free"] >> i & 1]
    z = np.abs(best["k16"][free] - c["k16"][free]) / best["std_dev"][free]
    print(f"{model_name}: rms {best['rms']:.3e} px, |k - k_gen| / std_dev at most {z.max():.2f}, fx {best['k16'][0]:.6f} fy {best['k16'][1]:.6f}")
    assert best["rms"] < 2.0 ** -13
    assert z.max() < 6.0
    assert abs(best["k16"][0] - cc.FX) < 1e-3 and abs(best["k16"][1] - cc.FY) < 1e-3
