#!/usr/bin/env python3
"""The figure behind FID_BUILD_ROBUST_MEASURED_PX and FID_BUILD_ROBUST_RECOMMENDED_PX (include/fid_abi.h): the largest err -- the
largest corner distance of an observation -- at the minimum of the PLAIN build, by the NumPy restatement
(tests/map_build_restatement.py), over the truthful cases of tests/map_build_cases.py and over ten rendered views of a two-wall scene
whose corners the CPU oracle detects (tests/test_gpu_map_build.py's end-to-end scene; the device's detector returns the oracle's
corners bit for bit, which the parity tests hold).  No GPU.  The recommendation is ten times the largest, rounded up to half a pixel.

    python tools/map_build_inlier_px.py"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import map_build_cases as mc  # noqa: E402
import map_build_restatement as mb  # noqa: E402


def largest_err(best) -> float:
    """The largest err of an observation at a restatement result's parameters."""
    r = best["problem"].res(best["x"]).reshape(-1, 4, 2)
    return float(np.sqrt((r * r).sum(-1)).max(axis=1).max())


def rendered_case():
    """Ten rendered 640 x 480 views of the two-wall scene of 8 markers, detected by the oracle, as a map_build_cases case."""
    import oracle
    from aruco_map_cases import K as K_MAP, corner_of_two_walls, look_at
    from fiducials_amd import synth
    from fiducials_amd.dictionary import get_predefined_dictionary
    scene = corner_of_two_walls(4, 4, first_id=20)
    spec = [(float(e["len"]), e["R"], e["t"]) for e in scene]
    rng = np.random.default_rng(31)
    d = get_predefined_dictionary(6)
    views, poses = [], []
    for i in range(10):
        pos = np.array([rng.uniform(0.55, 0.8), rng.uniform(-0.05, 0.3), rng.uniform(0.55, 0.8)])
        R, t = look_at(pos, np.array([0.15, 0.1, 0.15]))
        ids, corners = oracle.detect(synth.make_aruco_board_frame(d, scene["id"], spec, K_MAP, R, t, 300 + i, 640, 480).image, d)
        views.append((np.asarray(corners, np.float32).reshape(-1, 4, 2), np.asarray(ids, np.int32)))
        poses.append(np.concatenate([mb.rotation_vector(R), t]))
    k16 = np.zeros(16)
    k16[:4] = K_MAP[0, 0], K_MAP[1, 1], K_MAP[0, 2], K_MAP[1, 2]
    return dict(model=0, k16=k16, views=views, fixed=scene[:1], fiducial_len=0.125, len_override=None, min_views=2, true_markers=mc._true_markers(scene), poses=poses)


def rendered_err() -> float:
    return largest_err(mc.reference_of(rendered_case())["best"])


def recommended(measured_px: float) -> float:
    return math.ceil(10.0 * measured_px * 2.0) / 2.0


def main():
    worst = 0.0
    for name in mc.CASES:
        e = largest_err(mc.reference(name)["best"])
        worst = max(worst, e)
        print(f"{name}: {e:.4f} px", flush=True)
    r = rendered_err()
    print(f"rendered views: {r:.4f} px")
    worst = max(worst, r)
    print(f"largest: {worst:.4f} px; recommended inlier_px: {recommended(worst)}")


if __name__ == "__main__":
    main()
