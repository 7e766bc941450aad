"""The trimmed map build's reference against itself (tests/map_build_robust_restatement.py, tests/map_build_robust_cases.py), on the
CPU: every case flags exactly what was planted, keeps clear of every threshold, builds the map of the scene without the fault, and
the plain build of the faulty scene is visibly wrong.  Also the library's new symbol and the size of its record."""
import ctypes as C
import os

import numpy as np
import pytest

import map_build_cases as mc
import map_build_restatement as mb
import map_build_robust_cases as rc
import map_build_robust_restatement as mbr

# MEASURED HERE (the figures this file prints), restatement against restatement: on `swap`, `largest` and `moved` the plain build's worst
# marker ends 197, 27 and 44 mm from where the scene without the fault puts it, the trimmed build's at most 3e-6 mm.  The bounds
# asserted: the plain build is off by more than LARGEST_PLAIN_OFF_M on each, and by more than PLAIN_OVER_ROBUST times the trimmed build.
LARGEST_PLAIN_OFF_M = 1e-2
PLAIN_OVER_ROBUST = 1e4
FAULTS_THAT_MOVE_THE_PLAIN_MAP = ("swap", "largest", "moved")


def without_fault(c):
    """The case's views with the planted and the collateral observations taken out (a view may end empty)."""
    out = []
    gone = set(c["planted"]) | set(c["collateral"])
    for v, (corners, ids) in enumerate(c["views"]):
        keep = [p for p in range(len(ids)) if (v, p) not in gone]
        out.append((np.asarray(corners)[keep].reshape(-1, 4, 2), np.asarray(ids)[keep]))
    return out


def displacement(t_by_id, truth_t_by_id) -> float:
    """The largest distance between a marker's place and the truthful one, over the markers both hold."""
    common = set(t_by_id) & set(truth_t_by_id)
    return max(float(np.linalg.norm(np.asarray(t_by_id[i]) - np.asarray(truth_t_by_id[i]))) for i in common)


def truthful(c):
    """The plain restatement on the scene without the fault, from the rule's start and from the generating poses (the keep rule's two
    starts): reference_of's dict."""
    return mc.reference_of(dict(c, views=without_fault(c)))


@pytest.mark.parametrize("name", rc.CASES + (rc.WALL,))
def test_flags_exactly_the_planted_observations_and_builds_the_truthful_map(name):
    c, ref = rc.case(name), rc.reference(name)
    out = ref["out"]
    fl, ol = rc.flagged(out)
    print(f"{name}: rounds {out['rounds']} stable {out['stable']} planted {len(c['planted'])} collateral {len(c['collateral'])} outliers {len(ol)} left out {len(fl - ol)} "
          f"two-start gap {ref['gap']:.1e}")
    assert fl == set(c["planted"]) | set(c["collateral"]), (sorted(fl - set(c["planted"])), sorted(set(c["planted"]) - fl))
    assert ol <= set(c["planted"])
    thr0, e0 = out["first_set"]
    print(f"  first set at {thr0}: largest admitted {max([e for e in e0.values() if e <= thr0] + [-1]):.3f}, smallest refused {min([e for e in e0.values() if e > thr0] + [np.inf]):.3f}")
    for thr, es in out["history"]:
        near = [e for e in es.values() if thr / 2 < e < 2 * thr]
        print(f"  round at {thr}: largest admitted {max([e for e in es.values() if e <= thr] + [-1]):.3f}, smallest refused {min([e for e in es.values() if e > thr] + [np.inf]):.3f}")
        assert not near, near
    for e, thr in list(out["start_decisions"]) + [(e, thr0) for e in e0.values()]:  # under the start: map_robust_cases' 1 % clearance
        assert abs(e - thr) > 0.01 * thr, (e, thr)
    assert mbr.band_clear(out)
    assert ref["gap"] <= mc.KEEP_GAP and ref["kept"]
    # the map of the scene without the fault, at test_gpu_map_build's parameter bar
    tr = truthful(c)
    assert tr["kept"], tr["gap"]
    tb_, best = tr["best"], ref["best"]
    assert sorted(tb_["mposes"]) == sorted(best["mposes"]) and tb_["used"] == best["used"]
    t = max(10.0 * max(tr["gap"], ref["gap"]), 1e-9)
    x_rob = tb_["problem"].pack({tb_["slot"][i]: best["mposes"][i] for i in best["mposes"]}, [best["vposes"][v] for v in best["used"]])
    z = np.abs(x_rob - tb_["x"]) / (2.0 * np.sqrt(2.0 * t * tb_["dof"]) * tb_["std"])
    print(f"  against the scene without the fault: parameters {z.max():.3e} of the bar, cost {best['cost'] / tb_['cost'] - 1:.1e}")
    assert z.max() <= 1.0


@pytest.mark.parametrize("name", FAULTS_THAT_MOVE_THE_PLAIN_MAP)
def test_the_plain_build_of_the_faulty_scene_is_visibly_wrong(name):
    c, ref = rc.case(name), rc.reference(name)
    tr = truthful(c)["best"]
    place = lambda poses: {i: p[3:] for i, p in poses.items()}
    plain = mb.build(c["model"], c["k16"], c["views"], c["fixed"], c["fiducial_len"], len_override=c["len_override"], min_views=c["min_views"])
    d_plain, d_rob = displacement(place(plain["mposes"]), place(tr["mposes"])), displacement(place(ref["best"]["mposes"]), place(tr["mposes"]))
    print(f"{name}: the worst marker is off by {d_plain * 1e3:.3f} mm in the plain build, {d_rob * 1e3:.2e} mm in the trimmed one (factor {d_plain / max(d_rob, 1e-300):.1e})")
    assert d_plain > LARGEST_PLAIN_OFF_M
    assert d_plain > PLAIN_OVER_ROBUST * d_rob


def _inlier_px_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("map_build_inlier_px", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "map_build_inlier_px.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_recommended_inlier_px_is_ten_times_the_measured_err_rounded_up_to_half_a_pixel():
    """tools/map_build_inlier_px.py makes the measurement (the largest err at the plain minimum over map_build_cases.CASES and ten
    rendered views).  Here its deciding part is made again: the rendered views, which give the header's figure, and three of the
    generated cases, which stay below it; and the rule."""
    from fiducials_amd import _lib
    tool = _inlier_px_tool()
    rendered = tool.rendered_err()
    generated = max(tool.largest_err(mc.reference(name)["best"]) for name in ("views16", "model_rational", "corner"))
    print(f"largest err at the plain minimum: {rendered:.4f} px over the ten rendered views, {generated:.4f} px over three generated cases (header: {_lib.BUILD_ROBUST_MEASURED_PX})")
    assert abs(rendered - _lib.BUILD_ROBUST_MEASURED_PX) <= 1e-3 and generated <= rendered
    assert _lib.BUILD_ROBUST_INLIER_PX == tool.recommended(_lib.BUILD_ROBUST_MEASURED_PX) == rc.INLIER_PX


def test_why_the_first_set_round_0_over_every_kept_observation():
    """The feature was first specified with round 0 solving over EVERY kept observation (build_robust(first_set=False)); the header
    admits a first set under the start instead.  What the first meaning does on three of the cases, at the recommended inlier_px:
    the solve over everything spreads each gross error over the truthful observations of the same marker and view, whose err then
    stands AT the threshold -- on `moved` and `swap` the largest admitted and smallest refused err of round 0 are within 3 % of
    inlier_px on both sides, so which truthful observation is trimmed is a matter of rounding, no case could pass the keep
    condition, and the result needs three solves; on `largest` five truthful observations end as OUTLIER.  With the first set each of
    the three settles in one round with every err of a round below inlier_px / 7 or above 3 inlier_px."""
    for name in ("moved", "swap", "largest"):
        c = rc.case(name)
        lit, hdr = rc.run(c, first_set=False), rc.reference(name)["out"]
        thr, es = lit["history"][0]
        adm, ref_ = max(e for e in es.values() if e <= thr), min(e for e in es.values() if e > thr)
        _, ol = rc.flagged(lit)
        print(f"{name}: round 0 over everything: largest admitted {adm:.2f} px, smallest refused {ref_:.2f} px (inlier_px {thr}); rounds {lit['rounds']}, "
              f"truthful observations called OUTLIER {len(ol - set(c['planted']))}; with the first set: rounds {hdr['rounds']}")
        assert not mbr.band_clear(lit) and thr / 2 < adm and ref_ < 2 * thr  # (truthful errs inside the band on both sides)
        assert lit["rounds"] > hdr["rounds"] == 1
        for t, e in hdr["history"]:
            assert all(x < t / 7 or x > 3 * t for x in e.values())
    assert len(rc.flagged(rc.run(rc.case("largest"), first_set=False))[1] - set(rc.case("largest")["planted"])) == 5


def test_the_library_has_the_entry_point_and_the_record_s_size():
    from fiducials_amd import _lib
    L = C.CDLL(_lib.lib_path())
    assert hasattr(L, "fid_build_map_robust_cam")
    assert _lib.BUILD_ROBUST_OUT_DTYPE.itemsize == 40 and C.sizeof(_lib.FidBuildRobustOpts) == 16
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fid_abi.h")) as fh:
        text = fh.read()
    body = re.search(r"typedef struct fid_build_robust_out \{(.*?)\} fid_build_robust_out;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == list(_lib.BUILD_ROBUST_OUT_DTYPE.names)
    assert sum(4 if t == "int32_t" else 8 for t, _ in fields) == _lib.BUILD_ROBUST_OUT_DTYPE.itemsize
    assert ("FID_BUILD_OBS_NOT_KEPT 0" in text and "FID_BUILD_OBS_INLIER 1" in text and "FID_BUILD_OBS_OUTLIER 2" in text and "FID_BUILD_OBS_LEFT_OUT 3" in text)
    assert (_lib.OBS_NOT_KEPT, _lib.OBS_INLIER, _lib.OBS_OUTLIER, _lib.OBS_LEFT_OUT) == (0, 1, 2, 3)
