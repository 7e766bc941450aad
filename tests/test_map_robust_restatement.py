"""The consensus map pose without a GPU: the NumPy restatement (tests/map_robust_restatement.py) over the planted cases of
tests/map_robust_cases.py -- every case meets its keep conditions, which are conditions on the inputs --, the pieces of the
restatement against what they must reproduce, and the C-ABI: the built library exports the two entry points and the records have
the size the C compiler gives the structs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import aruco_map_cases as mc
import camera_model_cases as cm
import map_robust_cases as rc
import map_robust_restatement as rr
from fiducials_amd import _lib
from fiducials_amd.detector import MAP_ROBUST_DTYPE, map_robust_outlier_ids, map_robust_outlier_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(rc.cases()))
def test_case_is_kept(name):
    """The restatement recovers the planted set, every decision clears its threshold by > 1 %, the best two scores differ."""
    r = rc.restated(name)
    c = rc.cases()[name]
    print(name, "status", r["status"], "used", len(r["used"]), "inliers", len(r["inliers"]), "rounds", r["rounds"], "stable", r["stable"],
          "score", r["score"])
    if c.planted is not None:
        assert r["stable"] == 1 and 1 <= r["rounds"] <= rr.SOLVES
        assert max(r["errs"][j] for j in r["inliers"]) <= c.inlier_px
        out = [r["errs"][j] for j in r["eligible"] if j not in r["inliers"]]
        assert not out or min(out) > c.inlier_px


def test_wrong_markers_are_far_from_the_threshold():
    """An outlier of a planted case is shifted by >= 25 px or turned a quarter turn (its side length: 11 px on the smallest
    markers here, those of the 256-marker grids): more than 2.5 times inlier_px from where the map and the returned pose put it."""
    for name, c in rc.cases().items():
        r = rc.restated(name)
        if c.planted is None:
            continue
        for j in r["eligible"]:
            if j not in r["inliers"]:
                assert r["errs"][j] > 2.5 * c.inlier_px, (name, j, r["errs"][j])


def test_one_marker_pose_gives_an_exact_view_back():
    """Undistort, Heckbert's homography, the pose from it, composed with the map place: exact corners of a marker anywhere in the
    map give the generating pose back, under every camera model."""
    e = mc.planar_board("oblique5")
    P = mc.object_points(e).reshape(-1, 4, 3)
    R, t = rc._pose(3, "oblique5", tz_range=(0.9, 1.5))
    for model, D in ((cm.PLUMB_BOB, tuple(mc.D_NONZERO)), (cm.RATIONAL, cm.SETS["prism12"][1]), (cm.EQUIDISTANT, cm.SETS["fe_kb"][1])):
        for k in range(len(e)):
            img = cm.project(model, mc.K, D, R, t, P[k])
            Rh, th = rr.one_marker_pose(model, mc.K, D, P[k], img)
            # (five fixed-point iterations of the undistortion leave ~1e-9 at these distortions)
            assert np.abs(Rh - R).max() < 1e-6 and np.abs(th - t).max() < 1e-6, (model, k)


def test_lower_median_and_ties():
    """Element (m - 1) / 2 of the ascending list; the hypotheses are the 64 of largest area, the lower k first among equals."""
    c = rc.cases()["grid65"]
    r = rc.restated("grid65")
    assert len(r["scores"]) == rr.HYPOTHESES and len(r["eligible"]) == 65
    areas = [rc._area(c.corners[m].astype(np.float64)) for m in r["used"]]
    small = int(np.argmin(areas))
    assert small == 64 and small not in r["scores"]
    # with 65 hypotheses the smallest marker (its corners are exact) would win
    what_if = rc.restate(c, hypotheses=65)
    assert what_if["hypothesis"] == r["used"][small] and what_if["hypothesis"] != r["hypothesis"]


def test_readmission_case_readmits():
    r = rc.restated("readmission")
    assert r["rounds"] >= 2 and set(r["inliers"]) - set(r["I0"]), (r["rounds"], r["I0"], r["inliers"])


def test_four_solves_case_takes_four():
    """The search for a case that ENDS at the limit (stable = 0) over readmission_case(seed), seeds 1..299, inlier_px 0.45 / 0.6 /
    0.8 found none among the kept ones: a set that still changes after four solves has a marker near the threshold, which the 1 %
    keep condition rejects.  Two kept cases take all four solves and are stable at the fourth; this is one of them."""
    r = rc.restated("four_solves")
    assert r["rounds"] == rr.SOLVES and r["stable"] == 1


def test_used_markers_bookkeeping():
    c = rc.cases()["bookkeeping"]
    r = rc.restated("bookkeeping")
    assert r["used"] == [0, 2, 4, 6, 8, 9, 10] and r["n_over"] == 0
    assert tuple(r["used"][k] for k in r["inliers"]) == c.planted == (0, 2, 4, 6, 8, 10)
    r = rc.restated("grid257")
    assert len(r["used"]) == 256 and r["n_over"] == 1


def test_outlier_helpers():
    rec = np.zeros(1, MAP_ROBUST_DTYPE)[0]
    rec["n_used"] = 70
    rec["outlier_mask"] = [1 << 3, 1 << 2, 0, 0]
    assert map_robust_outlier_positions(rec).tolist() == [3, 66]
    ids = [500] + list(range(100, 135)) + [7, 7] + list(range(135, 170))  # 500 is not in the map, 7 is seen twice
    assert map_robust_outlier_ids(rec, ids, list(range(0, 400))).tolist() == [103, 166]
    with pytest.raises(ValueError):
        map_robust_outlier_ids(rec, ids[:-1], list(range(0, 400)))


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_library_exports_the_robust_entry_points():
    L = _lib.load()
    for s in ("fid_map_pose_robust_cam", "fid_map_pose_robust_last_cam"):
        assert hasattr(L, s), s


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "fid_abi.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(fid_map_robust_out), sizeof(fid_map_robust_opts), offsetof(fid_map_robust_out, score),
           offsetof(fid_map_robust_out, outlier_mask), offsetof(fid_map_robust_out, outlier_index), offsetof(fid_map_robust_opts, min_markers),
           FID_MAP_ROBUST_HYPOTHESES, FID_MAP_ROBUST_SOLVES);
    return 0;
}
"""


def test_record_sizes_are_the_c_compilers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler (the host tools need one)"
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.check_call([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")])
    got = [int(v) for v in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.split()]
    dt = MAP_ROBUST_DTYPE
    assert got == [dt.itemsize, C.sizeof(_lib.FidMapRobustOpts), dt.fields["score"][1], dt.fields["outlier_mask"][1], dt.fields["outlier_index"][1],
                   _lib.FidMapRobustOpts.min_markers.offset, _lib.MAP_ROBUST_HYPOTHESES, _lib.MAP_ROBUST_SOLVES], got
    assert (rr.HYPOTHESES, rr.SOLVES, rr.MAX_USED) == (_lib.MAP_ROBUST_HYPOTHESES, _lib.MAP_ROBUST_SOLVES, _lib.MAP_MAX_USED)
