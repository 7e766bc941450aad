"""Views with planted faults for the trimmed map build (tests/test_map_build_robust_restatement.py on the CPU,
tests/test_gpu_map_build_robust.py on the device): tests/map_build_cases.py's truthful noisy scenes, and in them

  swap            two ids swapped in one view
  largest         a wrong id whose observation is the LARGEST-area one of that marker (the plain start places the marker from it)
  moved           a fiducial moved by 10 cm for the last third of its views: the minority is flagged
  false_id        an id that no fiducial carries, seen in two views at unrelated places
  shifted_view    one view with every corner shifted by 30 px, each in a direction of its own (a common shift is a camera rotation)
  clean           nothing planted
  wall            two wrong ids per view on a 32-marker wall with 64 views
  swap_<model>    `swap` under each of the three camera models
  few_views       min_views 3, a marker kept by three views of which one is wrong: trimming takes it to FEW_VIEWS
  many_views      (beyond the list the feature was specified with) three markers in 72 views, two ids swapped in one: a marker has more
                  than FID_BUILD_ROBUST_HYPOTHESES hypotheses, so the 64 of largest area are chosen -- by k_pose's fiducial_area on the
                  device, by map_build_restatement.area here

A set that does not settle in four rounds is NOT here: none could be constructed on the CPU (every case above settles in one round; a
set oscillates only where an observation sits at the threshold, which the keep condition below excludes).

A case is (views, planted, collateral): planted = the observations {(view, list position)} that are wrong; collateral = truthful
observations that the fault takes out of the solve with it (few_views: the two truthful observations of the marker that falls
under min_views).  An observation counts as FLAGGED where its state is OUTLIER or LEFT_OUT: it is kept and does not enter the
returned solve.  The tests hold flagged == planted + collateral, and OUTLIER inside planted: nothing truthful is ever called an
outlier.  Two faults are flagged as LEFT_OUT, not OUTLIER, and why: shifted_view -- the consensus pose of a view whose every corner
is wrong does not exist, the view is NO_START and none of its observations ever has an err; false_id -- of two observations that
contradict each other the start follows one (the lower view on a tie of the scores), the other is the OUTLIER, and the marker, left
with one view, is FEW_VIEWS: nothing says which of the two was wrong, and neither enters the map.

THE KEEP CONDITION.  A case is kept only if in the restatement, in every round, no observation has err in (inlier_px / 2, 2
inlier_px): set membership is discrete, and the device and NumPy can only be compared where rounding cannot move an observation
across the line.  The decisions made under the START (inside the consensus pose of a view, and the first set) compare an err with a
threshold at poses that both sides compute as minima of the same small problems (tests/test_gpu_map_build_robust.py holds the
device's err under its start to the restatement's within a tenth of the clearance; measured 1e-7 to 3e-5 px); there every err must clear its
threshold by more than 1 %, tests/map_robust_cases.py's rule for the consensus pose.  (A truthful err under the start may well lie
between inlier_px / 2 and inlier_px: the start is a chain of single-marker poses, on the 32-marker wall up to 11.6 px off.)
tests/test_map_build_robust_restatement.py asserts both for every case; map_build_robust_restatement.band_clear is the rule.

INLIER_PX is the header's recommended value (FID_BUILD_ROBUST_RECOMMENDED_PX); MIN_VIEWS_PLACE 2."""
from __future__ import annotations

import functools

import numpy as np

import camera_model_cases as cmc
import map_build_cases as mc
import map_build_robust_restatement as mbr
from aruco_map_cases import NOISE_PX, fid_corners, grid_board

INLIER_PX = 13.5
MIN_VIEWS_PLACE = 2
CASES = ("swap", "largest", "moved", "false_id", "shifted_view", "clean", "swap_plumb_bob", "swap_rational", "swap_equidistant", "few_views", "many_views")
WALL = "wall"
FALSE_ID = 77


def _copy(views):
    return [(np.array(c, np.float32), np.array(i, np.int32)) for c, i in views]


def _derive(base, views, planted, **kw):
    c = dict(base)
    c.update(views=views, planted=frozenset(planted), collateral=frozenset(kw.pop("collateral", ())), truthful=base["views"], **kw)
    return c


def _swap(base, v):
    """The ids of the first two markers of view v that are not fixed, swapped."""
    views = _copy(base["views"])
    ids = views[v][1]
    free = [p for p, i in enumerate(ids) if int(i) not in set(base["fixed"]["id"])][:2]
    ids[free[0]], ids[free[1]] = ids[free[1]], ids[free[0]]
    return _derive(base, views, {(v, free[0]), (v, free[1])})


def _area(c):
    return mbr.mb.area(c)


@functools.lru_cache(maxsize=None)
def case(name: str):
    if name == "clean":
        return _derive(mc.case("views16"), _copy(mc.case("views16")["views"]), set())
    if name == "swap":
        return _swap(mc.case("views16"), 5)
    if name.startswith("swap_"):
        return _swap(mc.case("model_" + name[5:]), 2)
    if name == "largest":
        # the marker m and the observation (v, p) of another marker in a view without m whose area exceeds every area of m
        base = mc.case("views16")
        views = _copy(base["views"])
        fixed = set(int(i) for i in base["fixed"]["id"])
        for m in sorted(set(int(i) for _, ids in views for i in ids) - fixed):
            own = max(_area(c[p]) for c, ids in views for p in range(len(ids)) if ids[p] == m)
            cands = [(_area(c[p]), v, p) for v, (c, ids) in enumerate(views) if m not in ids for p in range(len(ids)) if int(ids[p]) not in fixed]
            if cands and max(cands)[0] > own:
                _, v, p = max(cands)
                views[v][1][p] = m
                return _derive(base, views, {(v, p)}, attacked=m)
        raise AssertionError("no marker can be attacked")
    if name == "moved":
        base = mc.case("views16")
        views = _copy(base["views"])
        model, k16 = base["model"], base["k16"]
        K = np.array([[k16[0], 0, k16[2]], [0, k16[1], k16[3]], [0, 0, 1.0]])
        m = 3
        e = base["entries"][base["entries"]["id"] == m][0]
        seen = [v for v, (_, ids) in enumerate(views) if m in ids]
        late = seen[len(seen) - len(seen) // 3:]
        rng = np.random.default_rng(20261201)
        planted = set()
        for v in late:
            p = int(np.nonzero(views[v][1] == m)[0][0])
            P = fid_corners(e["len"]) @ e["R"].T + e["t"] + e["R"] @ np.array([0.1, 0.0, 0.0])
            uv = cmc.project(model, K, list(k16[4:]), cmc.rodrigues(base["poses"][v][:3]), base["poses"][v][3:], P)
            views[v][0][p] = (uv + rng.uniform(-NOISE_PX, NOISE_PX, size=uv.shape)).astype(np.float32)
            planted.add((v, p))
        return _derive(base, views, planted, moved=m)
    if name == "false_id":
        base = mc.case("views16")
        views = _copy(base["views"])
        planted = set()
        for v, (dx, dy) in ((4, (37.0, -61.0)), (11, (-83.0, 45.0))):
            c, ids = views[v]
            views[v] = (np.concatenate([c, c[-1:] + np.array([dx, dy], np.float32)]), np.concatenate([ids, np.array([FALSE_ID], np.int32)]))
            planted.add((v, len(ids)))
        return _derive(base, views, planted)
    if name == "shifted_view":
        base = mc.case("views16")
        views = _copy(base["views"])
        v = 9
        rng = np.random.default_rng(20261202)
        ang = rng.uniform(0, 2 * np.pi, size=views[v][0].shape[:2])
        views[v] = ((views[v][0] + 30.0 * np.stack([np.cos(ang), np.sin(ang)], -1)).astype(np.float32), views[v][1])
        return _derive(base, views, {(v, p) for p in range(len(views[v][1]))}, shifted=v)
    if name == "few_views":
        base = mc.case("views16")
        views = _copy(base["views"])
        m = 6
        seen = [v for v, (_, ids) in enumerate(views) if m in ids]
        for v in seen[2:]:  # two truthful observations stay
            keep = views[v][1] != m
            views[v] = (views[v][0][keep], views[v][1][keep])
        fixed = set(int(i) for i in base["fixed"]["id"])
        v = next(v for v in range(len(views)) if v not in seen[:2] and len(views[v][1]) >= 3)
        p = next(p for p, i in enumerate(views[v][1]) if int(i) not in fixed)
        views[v][1][p] = m
        truthful = _copy(views)
        truthful[v] = (np.delete(truthful[v][0], p, axis=0), np.delete(truthful[v][1], p))
        collateral = {(u, int(np.nonzero(views[u][1] == m)[0][0])) for u in seen[:2]}
        c = _derive(base, views, {(v, p)}, collateral=collateral, min_views=3, thinned=m)
        c["truthful"] = truthful
        return c
    if name == "many_views":
        e = grid_board(3, 3)
        views, poses = mc.wall_views(e, 72, "plumb_bob", 700, dist=(0.5, 0.8))
        assert sum(1 for _, ids in views if 1 in ids) > mbr.HYPOTHESES and sum(1 for _, ids in views if 2 in ids) > mbr.HYPOTHESES
        return _swap(mc._case(e, views, poses, "plumb_bob", [0]), 5)
    if name == WALL:
        e = grid_board(32, 8)
        views, poses = mc.wall_views(e, 64, "plumb_bob", 500, dist=(0.9, 1.1), spread=0.9, grid=(8, 8), min_area=300.0)
        base = mc._case(e, views, poses, "plumb_bob", [0])
        views = _copy(views)
        rng = np.random.default_rng(20261203)
        planted = set()
        for v, (c, ids) in enumerate(views):
            free = [p for p, i in enumerate(ids) if int(i) != 0]
            absent = [i for i in range(1, 32) if i not in ids]
            if len(free) < 6 or len(absent) < 2:
                continue
            for p, i in zip(rng.choice(free, 2, replace=False), rng.choice(absent, 2, replace=False)):
                ids[p] = i
                planted.add((v, int(p)))
        return _derive(base, views, planted)
    raise KeyError(name)


def run(c, views=None, **kw):
    args = dict(len_override=c["len_override"], min_views=c["min_views"], min_views_place=MIN_VIEWS_PLACE)
    args.update(kw)
    return mbr.build_robust(c["model"], c["k16"], c["views"] if views is None else views, c["fixed"], c["fiducial_len"], INLIER_PX, **args)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """The restatement's answer with the two-start figures of map_build_cases.reference_of, the second start being the generating poses
    on the last solve's observations -> dict(best, gap, gap_cov, gap_rms, out)."""
    c = case(name)
    out = run(c, second_start=(c["true_markers"], dict(enumerate(c["poses"]))))
    a, g = out, out["second"]
    gap = abs(a["cost"] - g["cost"]) / min(a["cost"], g["cost"])
    ids = sorted(a["cov"])
    da = np.array([np.diag(a["cov"][i]) for i in ids]).reshape(-1)
    dg = np.array([np.diag(g["cov"][i]) for i in ids]).reshape(-1)
    best = a if a["cost"] <= g["cost"] else g
    return dict(best=best, gap=gap, gap_cov=float(np.max(np.abs(da - dg) / dg)) if len(dg) else 0.0, gap_rms=abs(a["rms"] - g["rms"]) / g["rms"], out=out,
                kept=gap <= mc.KEEP_GAP and mbr.band_clear(out))


def flagged(out):
    """({(v, p)} OUTLIER or LEFT_OUT, {(v, p)} OUTLIER)"""
    f, o = set(), set()
    for v, st in enumerate(out["obs_state"]):
        for p, s in enumerate(st):
            if s in (mbr.OBS_OUTLIER, mbr.OBS_LEFT_OUT):
                f.add((v, p))
            if s == mbr.OBS_OUTLIER:
                o.add((v, p))
    return f, o
