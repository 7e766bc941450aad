"""The map building reference against itself (tests/map_build_restatement.py, tests/map_build_cases.py), on the CPU: noise-free views
give the generating marker poses back, the selection and reachability rules, every case passes the keep rule, and the analytic
pieces -- the batch rotation, the file's angles -- agree with the complex step and with the map file's own reader."""
import numpy as np
import pytest

import camera_model_cases as cmc
import map_build_cases as mc
import map_build_restatement as mb
from aruco_map_cases import grid_board


def test_keep_and_plan():
    assert mb.keep([5, 7, 5, 9]) == ([1, 3], 0)
    assert mb.keep(list(range(70))) == (list(range(64)), 6)
    ids = lambda *a: (np.zeros((len(a), 4, 2), np.float32), np.array(a, np.int32))
    views = [ids(0, 1), ids(1, 2), ids(0, 1), ids(10, 11), ids(11, 10), ids(30), ids(1, 1, 2)]
    pl = mb.plan(views, [0], min_views=2)
    assert pl["ids"] == [0, 1, 2, 10, 11, 30] and pl["solve"] == [0, 1, 2]
    assert pl["mstatus"] == {0: mb.M_FIXED, 1: mb.M_SOLVED, 2: mb.M_SOLVED, 10: mb.M_UNREACHED, 11: mb.M_UNREACHED, 30: mb.M_FEW_VIEWS}
    assert pl["vstatus"] == [mb.V_USED, mb.V_USED, mb.V_USED, mb.V_UNREACHED, mb.V_UNREACHED, mb.V_FEW, mb.V_USED]
    assert pl["n_views"][1] == 3 and pl["n_views"][2] == 2  # (view 6 shows id 1 twice: left out of it)
    pl = mb.plan(views[:3], [0], min_views=3)
    assert pl["solve"] == [0, 1] and pl["mstatus"][2] == mb.M_FEW_VIEWS
    with pytest.raises(mb.TooManyMarkers):
        mb.plan([ids(*range(0, 64)), ids(*range(63, 127)), ids(*range(126, 130)), ids(*range(0, 64)), ids(*range(63, 127)), ids(*range(126, 130))], [0])


def test_batch_rotation_is_the_single_one_and_takes_the_complex_step():
    rng = np.random.default_rng(5)
    r = rng.uniform(-2, 2, (7, 3))
    R = mb.rodrigues_b(r)
    for k in range(7):
        assert np.abs(R[k] - cmc.rodrigues(r[k])).max() < 1e-15
    assert np.abs(mb.rodrigues_b(np.zeros((1, 3)))[0] - np.eye(3)).max() == 0
    h = 1e-30
    for j in range(3):
        rc = r.astype(np.complex128)
        rc[:, j] += 1j * h
        d = np.imag(mb.rodrigues_b(rc)) / h
        step = np.zeros(3)
        step[j] = 1e-6
        fd = (mb.rodrigues_b(r + step) - mb.rodrigues_b(r - step)) / 2e-6
        assert np.abs(d - fd).max() < 1e-8


@pytest.mark.parametrize("camera", ["plumb_bob", "rational", "equidistant"])
def test_noise_free_views_give_the_generating_markers(camera):
    e = grid_board(6, 3)
    views, poses = mc.wall_views(e, 5, camera, 123, dist=(0.6, 0.85), noise=0.0)
    c = mc._case(e, views, poses, camera, [0])
    a = mb.build(c["model"], c["k16"], c["views"], c["fixed"], c["fiducial_len"])
    assert a["rms"] < 2e-5  # (the corners are rounded to float32: 3e-5 px at 480)
    for i, p in a["mposes"].items():
        assert np.abs(p - c["true_markers"][i]).max() < 1e-6, (i, p, c["true_markers"][i])
    for v, p in a["vposes"].items():
        assert np.abs(p - c["poses"][v]).max() < 1e-6


def test_the_jacobian_against_central_differences_and_the_cost_of_the_start():
    c, ref = mc.case("corner"), mc.reference("corner")
    prob, x = ref["best"]["problem"], ref["rule"]["x0"]
    J = prob.jacobian(x)
    for j in range(0, len(x), 5):
        step = np.zeros(len(x))
        step[j] = 1e-6
        fd = (prob.res(x + step) - prob.res(x - step)) / 2e-6
        assert np.abs(J[:, j] - fd).max() < 1e-4 * max(1.0, np.abs(fd).max())
    assert ref["rule"]["cost"] <= ref["rule"]["start_cost"]
    # cov's blocks are those of the dense inverse
    cov, std, cost, dof = mb.covariance(prob, ref["best"]["x"])
    full = np.linalg.inv(J.T @ J) if False else np.linalg.inv(prob.jacobian(ref["best"]["x"]).T @ prob.jacobian(ref["best"]["x"])) * cost / dof
    for s, blk in cov.items():
        i = prob.col[s]
        assert np.abs(blk - full[i:i + 6, i:i + 6]).max() <= 1e-6 * np.abs(np.diag(blk)).max()


@pytest.mark.parametrize("name", mc.CASES + (mc.LARGE,))
def test_every_case_is_kept(name):
    ref = mc.reference(name)
    print(f"{name}: gap {ref['gap']:.2e} cov {ref['gap_cov']:.2e} rms {ref['gap_rms']:.2e} iterations {ref['rule']['iterations']} / {ref['given']['iterations']}")
    assert ref["kept"], ref["gap"]
    assert max(10 * ref["gap_cov"], 10 * ref["gap_rms"]) < 1e-3


def test_the_named_cases_are_what_they_say():
    pl = mc.reference("chain3_min1")["rule"]["plan"]
    assert [sorted(i for _, i in k) for k in pl["kept"]] == [[0, 1], [1, 2], [0, 1]] and pl["solve"] == [0, 1, 2]
    pl = mc.reference("chain3_min2")["rule"]["plan"]
    assert pl["solve"] == [0, 1] and pl["mstatus"][2] == mb.M_FEW_VIEWS and pl["vstatus"] == [0, 0, 0]
    pl = mc.reference("two_components")["rule"]["plan"]
    assert pl["mstatus"][10] == pl["mstatus"][11] == mb.M_UNREACHED and pl["vstatus"][4:] == [mb.V_UNREACHED] * 2
    for n in (10, 11, 21, 22, 127):
        assert len(mc.reference("size%d" % n)["rule"]["plan"]["solve"]) == n + 1
    with pytest.raises(mb.TooManyMarkers):
        c = mc.case(mc.TOO_MANY)
        mb.plan(c["views"], c["fixed"]["id"])
    pl = mc.reference("lists")["rule"]["plan"]
    assert pl["n_over"] == [0, 1, 16, 0] and len(pl["solve"]) == 64
    c = mc.case("mixed")
    assert (c["views"][2][1] == 3).sum() == 2 and len(c["fixed"]) == 2
