"""k_approx (fid_kernels.hip) rejects a contour as soon as new_count + top > K4_MAX_RAW (= 9), checked before a slice is popped:
every slice still on the stack ends as at least one vertex of the raw polygon, and the clean-up pass drops at most one vertex per
two of its steps, so 10 raw vertices cannot end as the 4 of a candidate (9 can: 9 -> 4).  That bound is what lets the slice stack
be K4_STACK entries and nothing else.

Here: the NumPy restatement of the recursion in the kernel's order of work (tests/approx_restatement.py), without the bound
against oracle.approx_poly_dp -- so that the restatement is known to be the reference's algorithm -- and with it: the bound only
ever rejects contours whose raw polygon has more than K4_MAX_RAW vertices and whose polygon from the reference is no quad, leaves
the vertices of every other contour as they were, and the stack never holds more than 10 slices."""
import numpy as np

import oracle
from approx_restatement import approx_restated, gate_contours, random_closed_contours, source_define
from fiducials_amd.dictionary import get_predefined_dictionary
from fiducials_amd.synth import make_frame

MAX_RAW = source_define("K4_MAX_RAW")


def check(contours, rate):
    rejected = few = deepest = 0
    for c in contours:
        rej0, raw, v0, deep0 = approx_restated(c, rate)
        assert not rej0
        ref = oracle.approx_poly_dp(c, float(len(c)) * rate)
        assert np.array_equal(v0, ref), (len(c), v0, ref)  # the restatement is the reference's algorithm
        rej, raw1, v1, deep1 = approx_restated(c, rate, MAX_RAW)
        deepest = max(deepest, deep1)
        if rej:
            rejected += 1
            assert raw > MAX_RAW, (len(c), raw)
            assert len(ref) != 4, (len(c), raw, ref)  # the bound only takes what the reference does not make a quad of
        else:
            assert raw1 == raw and raw <= MAX_RAW and np.array_equal(v1, v0)
            few += 1
    assert deepest <= 10, deepest
    return rejected, few, deepest


def test_bound_on_random_closed_contours():
    rng = np.random.default_rng(11)
    cs = random_closed_contours(rng, 400)
    total_rej = total_few = 0
    for rate in (0.01, 0.03, 0.1):
        rej, few, _ = check(cs, rate)
        total_rej += rej
        total_few += few
    assert total_rej > 0 and total_few > 0  # both sides of the bound are really present


def test_bound_on_the_gate_contours_of_two_frames():
    d = get_predefined_dictionary("DICT_5X5_250")
    p = oracle.default_params()
    p.minMarkerPerimeterRate = 0.1  # (the node's default, as in the benchmark)
    for seed in (1000, 1001):
        fr = make_frame(d, seed=seed, width=1280, height=720, n_markers=12)
        cs = gate_contours(fr.image, p)
        assert len(cs) > 100
        rej, few, deepest = check(cs, p.polygonalApproxAccuracyRate)
        assert rej > 0 and few > 0


def test_the_kernels_stack_holds_the_bound():
    """The clean-up pass (approx.cpp) visits cnt vertices and skips the one behind each it drops: at most ceil(cnt / 2) go, so
    MAX_RAW + 1 vertices leave at least 5; and top <= MAX_RAW at a pop, MAX_RAW + 1 after its two pushes."""
    assert MAX_RAW == 9 and (MAX_RAW + 1) - (MAX_RAW + 2) // 2 > 4 and MAX_RAW - (MAX_RAW + 1) // 2 <= 4
    assert source_define("K4_STACK") >= MAX_RAW + 1
    assert "if (new_count + top > K4_MAX_RAW)" in open(__import__("approx_restatement").SRC).read()
