"""fid_build_map_robust_cam (include/fid_abi.h: "building the map from views that hold wrong detections") restated in NumPy, float64,
from the header's text: err, the candidates over the active observations, the robust start (a view by the consensus map pose of
tests/map_robust_restatement.py, a marker by the hypothesis of smallest lower-median err), the first set, the rounds, the states of the
observations.  A round's solve is tests/map_build_restatement.py's dense Levenberg-Marquardt on a Problem of the active observations.
It is the reference of tests/test_gpu_map_build_robust.py; no test functions and no GPU here.

Views, the camera (model, k16) and `fixed` are map_build_restatement's.  An observation is named (v, p): view v, LIST position p."""
from __future__ import annotations

import numpy as np

import camera_model_cases as cmc
import map_build_restatement as mb
import map_robust_restatement as mr
from calib_restatement import rotation_vector

SOLVES, HYPOTHESES = 4, 64
OBS_NOT_KEPT, OBS_INLIER, OBS_OUTLIER, OBS_LEFT_OUT = range(4)


def plan(kept, active, fixed_ids, min_views):
    """map_build_restatement.plan over the active observations.  kept: [[(p, id)]]; active: {(v, p)}.  FIXED / SOLVED stand for "in the
    solve"."""
    act = [[(p, i) for p, i in k if (v, p) in active] for v, k in enumerate(kept)]
    all_ids = sorted({i for k in kept for _, i in k})
    n_act = {i: sum(1 for k in act for _, j in k if j == i) for i in all_ids}
    fixed_ids = set(int(i) for i in fixed_ids)
    cand = {i for i in all_ids if i in fixed_ids or n_act[i] >= min_views}
    placed = {i for i in all_ids if i in fixed_ids}
    reached = [False] * len(kept)
    changed = True
    while changed:
        changed = False
        for v, k in enumerate(act):
            if not reached[v] and any(i in placed for _, i in k):
                reached[v] = changed = True
                placed |= {i for _, i in k if i in cand}
    mstatus = {i: mb.M_FIXED if i in fixed_ids else mb.M_FEW_VIEWS if i not in cand else mb.M_SOLVED if i in placed else mb.M_UNREACHED for i in all_ids}
    vstatus = [mb.V_USED if reached[v] else mb.V_FEW if not any(i in cand for _, i in k) else mb.V_UNREACHED for v, k in enumerate(act)]
    if len(placed) > mb.MAX_MARKERS:
        raise mb.TooManyMarkers(len(placed))
    return dict(ids=all_ids, mstatus=mstatus, vstatus=vstatus, solve=[i for i in all_ids if i in placed], reached=reached)


def err_of(model, k16, mpose, vpose, h, corners) -> float:
    """err: the largest corner distance under the marker pose (R, t) and the view pose (six)."""
    uv = mb.project_obs(model, k16, mpose[0][None], mpose[1][None], vpose[None, :3], vpose[None, 3:], np.array([h]))[0]
    d = uv - corners
    return float(np.sqrt((d * d).sum(axis=1)).max())


def robust_start(model, k16, split, kept, pl, fixed, lens, inlier_px, min_views_place):
    """-> (marker poses {id: (R, t)}, view poses {v: six}, views without a start, decisions [(err, threshold)] of the views' solves)."""
    K = np.array([[k16[0], 0, k16[2]], [0, k16[1], k16[3]], [0, 0, 1.0]])
    D = list(k16[4:])
    placed = {int(e["id"]): (np.asarray(e["R"], np.float64), np.asarray(e["t"], np.float64)) for e in fixed if int(e["id"]) in pl["solve"]}
    vposes, no_start, decisions, single = {}, set(), [], {}
    changed = True
    while changed:
        changed = False
        for v, k in enumerate(kept):
            if v in vposes or v in no_start or not pl["reached"][v] or not any(i in placed for _, i in k):
                continue
            entries = [dict(id=i, len=lens[i], R=placed[i][0], t=placed[i][1]) for i in sorted(placed) if i in pl["solve"]]
            r = mr.restate(model, K, D, entries, [i for _, i in k], np.stack([split[v][1][p] for p, _ in k]), inlier_px, 1)
            decisions += r["decisions"]
            changed = True
            if r["status"] != mr.OK or not np.isfinite(r["t"]).all():
                no_start.add(v)
                continue
            vposes[v] = np.concatenate([rotation_vector(r["R"]), r["t"]])
        for i in pl["solve"]:
            if i in placed:
                continue
            seen = [(v, p) for v in sorted(vposes) for p, j in kept[v] if j == i]
            if len(seen) < min_views_place:
                continue
            hyps = []
            for v, p in seen:
                if (v, p) not in single:
                    single[(v, p)] = mb.marker_pose(model, k16, split[v][1][p], lens[i])
                q = single[(v, p)]
                if not np.isfinite(q).all():
                    continue
                Rcm, Rcf = cmc.rodrigues(vposes[v][:3]), cmc.rodrigues(q[:3])
                hyps.append((-mb.area(split[v][1][p]), v, (Rcm.T @ Rcf, Rcm.T @ (q[3:] - vposes[v][3:]))))
            hyps = sorted(hyps, key=lambda t: t[:2])[:HYPOTHESES]
            best = None
            for _, hv, pose in hyps:
                e = sorted(err_of(model, k16, pose, vposes[v], mb.half(lens[i]), split[v][1][p]) for v, p in seen)
                score = e[(len(e) - 1) // 2]
                if np.isfinite(score) and (best is None or (score, hv) < best[:2]):
                    best = (score, hv, pose)
            if best is not None:
                placed[i] = best[2]
                changed = True
    return placed, vposes, no_start, decisions


def _records(prob, slot, used, solve_ids, x, sigma_px):
    """The part of map_build_restatement.build behind the solve."""
    cov, std, c, dof = mb.covariance(prob, x, sigma_px)
    r = prob.res(x).reshape(-1, 8)
    mrms = {i: float(np.sqrt((r[prob.os == slot[i]] ** 2).sum() / (4 * (prob.os == slot[i]).sum()))) for i in solve_ids if (prob.os == slot[i]).any()}
    vrms = {v: float(np.sqrt((r[prob.ov == u] ** 2).sum() / (4 * (prob.ov == u).sum()))) for u, v in enumerate(used)}
    mposes = {i: x[prob.col[slot[i]]:prob.col[slot[i]] + 6] for i in solve_ids if slot[i] in prob.col}
    vposes = {v: x[prob.nm + 6 * u:prob.nm + 6 * u + 6] for u, v in enumerate(used)}
    return dict(problem=prob, slot=slot, used=used, x=x, cost=c, cov={i: cov[slot[i]] for i in mposes}, std=std, dof=dof, rms=float(np.sqrt(c / (4 * len(prob.os)))),
                mrms=mrms, vrms=vrms, mposes=mposes, vposes=vposes, n_points=4 * len(prob.os), n_free=prob.n())


def build_robust(model, k16, views, fixed, fiducial_len, inlier_px, min_views_place: int = 1, len_override=None, min_views: int = 2, sigma_px: float = 0.0,
                 max_iter: int = 500, second_start=None, first_set: bool = True):
    """The reference answer of one call.  second_start = (marker poses {id: six}, view poses {v: six}): the LAST solve is run again
    from there (the two-start gap of map_build_cases' keep rule, on the final observation set).  first_set = False is NOT the header's
    meaning: round 0 then solves over every kept observation, as the feature was first specified; tests/
    test_map_build_robust_restatement.py shows with it why the header admits a first set under the start."""
    split = [mb.split_view(v) for v in views]
    kept = []
    for ids, _ in split:
        pos, _ = mb.keep(ids)
        kept.append([(p, int(ids[p])) for p in pos])
    all_obs = [(v, p) for v, k in enumerate(kept) for p, _ in k]
    id_of = {(v, p): i for v, k in enumerate(kept) for p, i in k}
    active = set(all_obs)
    fixed_ids = [int(i) for i in fixed["id"]]
    pl = plan(kept, active, fixed_ids, min_views)
    lens = mb.lengths(pl["ids"], fiducial_len, len_override, fixed)
    mpose, vpose, no_start, decisions = robust_start(model, k16, split, kept, pl, fixed, lens, inlier_px, min_views_place)
    mpose, vpose = dict(mpose), dict(vpose)
    fx = {int(e["id"]): (np.asarray(e["R"], np.float64), np.asarray(e["t"], np.float64)) for e in fixed}
    mvec = {}  # a solved marker's six parameters

    def errs():
        return {o: err_of(model, k16, mpose[id_of[o]], vpose[o[0]], mb.half(lens[id_of[o]]), split[o[0]][1][o[1]]) for o in all_obs
                if o[0] in vpose and id_of[o] in mpose}

    def admit(e, thr):
        return {o for o in all_obs if (e[o] <= thr if o in e else o in active)}

    def solve_over(pl, active, start=None):
        solve_ids = [i for i in pl["solve"] if i in mpose]
        slot = {i: s for s, i in enumerate(solve_ids)}
        used = [v for v in range(len(views)) if pl["reached"][v] and v in vpose and any((v, p) in active and i in slot for p, i in kept[v])]
        if not used:
            return None
        obs = [(u, slot[i], split[v][1][p]) for u, v in enumerate(used) for p, i in kept[v] if (v, p) in active and i in slot]
        prob = mb.Problem(model, k16, len(slot), {slot[i]: fx[i] for i in solve_ids if i in fx}, {slot[i]: mb.half(lens[i]) for i in solve_ids}, obs, len(used))
        if 8 * len(obs) < prob.n():
            return None
        if start is None:
            ms = {slot[i]: mvec[i] if i in mvec else np.concatenate([rotation_vector(mpose[i][0]), mpose[i][1]]) for i in solve_ids if slot[i] in prob.col}
            vs = [vpose[v] for v in used]
        else:
            ms = {slot[i]: np.asarray(start[0][i], np.float64) for i in solve_ids if slot[i] in prob.col}
            vs = [np.asarray(start[1][v], np.float64) for v in used]
        x0 = prob.pack(ms, vs)
        x, c, it = mb.lm(prob, x0, max_iter=max_iter)
        return prob, slot, used, solve_ids, x, it

    history = []  # per round: (threshold, {obs: err})
    e0 = errs()
    n_obs = len(e0)
    thr0 = inlier_px  # the first set
    if first_set:
        active = admit(e0, thr0)
        pl = plan(kept, active, fixed_ids, min_views)
    if not any(pl["reached"]):
        raise ValueError("no reached view")
    fin, rounds, stable = None, 0, 0
    for rnd in range(SOLVES):
        s = solve_over(pl, active)
        if s is None:
            if rnd == 0:
                raise ValueError("nothing to solve")
            break
        prob, slot, used, solve_ids, x, it = s
        for i in solve_ids:
            if slot[i] in prob.col:
                mvec[i] = x[prob.col[slot[i]]:prob.col[slot[i]] + 6].copy()
                mpose[i] = (cmc.rodrigues(mvec[i][:3]), mvec[i][3:].copy())
        for u, v in enumerate(used):
            vpose[v] = x[prob.nm + 6 * u:prob.nm + 6 * u + 6].copy()
        e = errs()
        history.append((inlier_px, e))
        fin = dict(prob=prob, slot=slot, used=used, solve_ids=solve_ids, x=x, it=it, pl=pl, active=set(active), err=e)
        rounds = rnd + 1
        nxt = admit(e, inlier_px)
        if nxt == active:
            stable = 1
            break
        if rnd + 1 == SOLVES:
            break
        active = nxt
        pl = plan(kept, active, fixed_ids, min_views)
        if not any(pl["reached"]):
            break
    pl, act = fin["pl"], fin["active"]
    mstatus = {i: (mb.M_NO_START if (s in (mb.M_FIXED, mb.M_SOLVED) and i not in fin["slot"]) else s) for i, s in pl["mstatus"].items()}
    vstatus = []
    for v in range(len(views)):
        if pl["reached"][v]:
            vstatus.append(mb.V_USED if v in fin["used"] else mb.V_NO_START)
        else:
            vstatus.append(pl["vstatus"][v])
    state = [np.zeros(len(ids), np.uint8) for ids, _ in split]
    err = [np.full(len(ids), -1.0) for ids, _ in split]
    for o in all_obs:
        v, p = o
        if o not in act:
            state[v][p] = OBS_OUTLIER
        elif id_of[o] in fin["slot"] and v in fin["used"]:
            state[v][p] = OBS_INLIER
        else:
            state[v][p] = OBS_LEFT_OUT
        if o in fin["err"]:
            err[v][p] = fin["err"][o]
    inl = [fin["err"][o] for o in all_obs if state[o[0]][o[1]] == OBS_INLIER]
    outl = [fin["err"][o] for o in all_obs if state[o[0]][o[1]] == OBS_OUTLIER and o in fin["err"]]
    rec = _records(fin["prob"], fin["slot"], fin["used"], fin["solve_ids"], fin["x"], sigma_px)
    out = dict(rounds=rounds, stable=stable, n_obs=n_obs, n_inliers=len(inl), n_outliers=sum(int((s == OBS_OUTLIER).sum()) for s in state),
               worst_inlier_px=max(inl) if inl else -1.0, best_outlier_px=min(outl) if outl else -1.0, obs_state=state, obs_err=err, mstatus=mstatus, vstatus=vstatus,
               marker_outliers={i: sum(1 for o in all_obs if id_of[o] == i and o not in act) for i in pl["ids"]},
               view_outliers=[sum(1 for o in all_obs if o[0] == v and o not in act) for v in range(len(views))], history=history, first_set=(thr0, e0),
               start_decisions=decisions,
               lens=lens, iterations=fin["it"], kept=kept, **rec)
    if second_start is not None:
        s2 = solve_over(pl, act, start=second_start)
        out["second"] = _records(s2[0], s2[1], s2[2], s2[3], s2[4], sigma_px)
    return out


def band_clear(out, lo: float = 0.5, hi: float = 2.0, start_clearance: float = 0.01) -> bool:
    """The keep condition: in every round no err lies in (threshold / 2, 2 threshold); under the start -- the consensus poses' own
    decisions and the first set -- every err clears its threshold by more than 1 %."""
    rounds = all(not (lo * thr < e < hi * thr) for thr, es in out["history"] for e in es.values())
    thr0, e0 = out["first_set"]
    start = all(abs(e - thr) > start_clearance * thr for e, thr in list(out["start_decisions"]) + [(e, thr0) for e in e0.values()])
    return rounds and start
