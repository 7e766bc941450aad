"""The rig pose restated in NumPy (tests/rig_restatement.py) on the CPU: its analytic Jacobian against central differences for each
camera model behind a non-trivial extrinsic, exact projections through a three-camera rig of mixed models giving the pose back, the
joint cost not rising from the start, the record's layout against the C struct, RigCamera.from_tf against a hand-computed case, and
the host class's test program building and printing its usage.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import aruco_map_cases as mc
import camera_model_cases as cm
import rig_cases as rc
import rig_restatement as rr
from fiducials_amd import _lib
from fiducials_amd.camera import Camera, RigCamera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("model_name", ["pb", "rat", "fe"])
def test_the_jacobian_equals_central_differences(model_name):
    """d(u, v) / d(rvec, tvec) through (R_c, t_c) and the camera's model: relative 1e-6 of the largest entry of its column."""
    cam = rc.make_cam(model_name, (0.07, -0.03, 0.02), (0.15, -0.25, 0.1))
    c = rc.case("three_models")
    P = mc.object_points(c.entries)
    p0 = np.concatenate([rr.rotvec(c.R), c.t])
    uv, J = rr.project([cam], np.zeros(len(P), int), p0, P, True)
    assert (uv[:, 0] > 0).all() and (uv[:, 0] < rc.W).all() and (uv[:, 1] > 0).all() and (uv[:, 1] < rc.H).all()
    h = 1e-6
    for j in range(6):
        e = np.zeros(6)
        e[j] = h
        num = (rr.project([cam], np.zeros(len(P), int), p0 + e, P) - rr.project([cam], np.zeros(len(P), int), p0 - e, P)) / (2 * h)
        rel = np.abs(J[:, :, j] - num).max() / np.abs(num).max()
        assert rel < 1e-6, (model_name, j, rel)
    # ... and the value is camera_model_cases' projection under the composed pose
    want = cm.project(cam.model, cam.K, cam.D, cam.R @ c.R, cam.R @ c.t + cam.t, P)
    assert np.abs(uv - want).max() < 1e-9


def test_exact_projections_through_a_mixed_rig_give_the_pose_back():
    c = rc.case("three_models")
    assert sorted(cam.model for cam in c.cams) == [cm.PLUMB_BOB, cm.RATIONAL, cm.EQUIDISTANT]
    r = rc.restated(c.name)
    assert r["n_markers"] == 14 and r["n_cameras"] == 3 and r["n_per_camera"][:3].tolist() == [4, 6, 4] and r["n_over"] == 0 and r["n_unposable"] == 0
    d = rc.dist(r["R"], r["tvec"], c.R, c.t)
    print("three models, exact projections (rounded to float): distance to the pose", d)
    assert d < 1e-5  # (float32 corners: 1e-5 px / 466 px at 1.2 m)
    assert np.abs(r["rig_R"] - r["R"].T).max() == 0 and np.abs(r["rig_t"] + r["R"].T @ r["tvec"]).max() < 1e-15


def test_the_joint_cost_does_not_rise_from_the_start():
    for c in rc.cases():
        r = rc.restated(c.name)
        assert r["costs"][-1] <= r["costs"][0], (c.name, r["costs"][0], r["costs"][-1])
        # every accepted step of the ladder is a descent or the ladder's end; the result is where the last evaluation was
        final = ((rr.project(c.cams, r["pcam"], np.concatenate([r["rvec"], r["tvec"]]), r["P"]) - r["img"]) ** 2).sum()
        assert abs(final - r["costs"][-1]) <= 1e-12 * max(final, 1.0)


def test_the_gather_rules_of_the_restatement():
    c = rc.case("two_cameras")
    ids = [c.ids[0].copy(), c.ids[1].copy()]
    corners = [c.corners[0].copy(), c.corners[1].copy()]
    base, over, bad = rr.gather(c.cams, c.entries, ids, corners)
    assert len(base) == 10 and over == 0 and bad == 0
    ids[0] = np.concatenate([ids[0], ids[0][:1], [999]])  # the first id twice in camera 0, and an id the map does not name
    corners[0] = np.concatenate([corners[0], corners[0][:1] + 40, corners[0][:1] + 80])
    used, over, bad = rr.gather(c.cams, c.entries, ids, corners)
    assert used == [u for u in base if u != (0, 0)] and (1, 3) in used  # (camera 1 still uses that id: list index 3 there)
    assert int(c.ids[1][3]) == int(c.ids[0][0])


def test_the_record_dtype_has_the_size_of_the_c_struct(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "fid_abi.h"\nint main(void) { printf("%zu %zu %d %d\\n", sizeof(fid_rig_pose_out), sizeof(fid_rig_camera), '
                   'FID_RIG_MAX_CAMERAS, FID_RIG_MAX_USED); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert [int(v) for v in out] == [_lib.RIG_POSE_DTYPE.itemsize, C.sizeof(_lib.FidRigCamera), _lib.RIG_MAX_CAMERAS, _lib.RIG_MAX_USED]
    assert _lib.RIG_MAX_CAMERAS == rr.MAX_CAMERAS and _lib.RIG_MAX_USED == rr.MAX_USED


def test_from_tf_inverts_the_transform():
    """A camera 0.2 m to the rig's left and 0.1 m up, turned 90 degrees about the rig's z: q = (0, 0, sin 45, cos 45).  The camera's
    axes in the rig are x_c = +y, y_c = -x, so R (rig -> camera) = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]] and t = -R xyz = (-0.1, 0.2, 0)
    for xyz = (0.2, 0.1, 0)."""
    cam = Camera(cm.PLUMB_BOB, rc.K, np.zeros(5))
    s = np.sqrt(0.5)
    got = RigCamera.from_tf([0.2, 0.1, 0.0], [0.0, 0.0, s, s], cam)
    assert np.abs(got.R - np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])).max() < 1e-15
    assert np.abs(got.t - np.array([-0.1, 0.2, 0.0])).max() < 1e-15
    assert got.camera.model == cm.PLUMB_BOB and np.array_equal(got.camera.K, rc.K)
    # a quaternion that is not normalised says the same rotation; the restatement's from_tf agrees
    again = RigCamera.from_tf([0.2, 0.1, 0.0], [0.0, 0.0, 3.0, 3.0], cam)
    assert np.abs(again.R - got.R).max() < 1e-15 and np.abs(again.t - got.t).max() < 1e-15
    R, t = rr.from_tf([0.2, 0.1, 0.0], [0.0, 0.0, s, s])
    assert np.abs(R - got.R).max() < 1e-15 and np.abs(t - got.t).max() < 1e-15
    with pytest.raises(_lib.FidError):
        RigCamera.from_tf([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], cam)
    with pytest.raises(_lib.FidError):
        RigCamera.from_tf([np.nan, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], cam)


def test_the_rendered_scene_is_one_the_reference_detects_completely():
    """synth.make_rig_frames' scene of test_gpu_rig_pose*.py: the oracle finds every rendered id in both cameras' frames, and camera c's
    frame is make_aruco_board_frame's under the pose (R_c R, R_c t + t_c)."""
    import oracle
    from fiducials_amd.dictionary import get_predefined_dictionary

    frames = rc.scene_frames()
    R, t = rc.scene_pose()
    assert len(frames) == 2
    for f, cam in zip(frames, rc.SCENE_RIG):
        oids, _ = oracle.detect(f.image, get_predefined_dictionary(mc.DICT))
        assert sorted(oids.tolist()) == sorted(f.ids.tolist()) and len(oids) == 6
        assert np.abs(f.R - cam.R @ R).max() < 1e-15 and np.abs(f.tvec - (cam.R @ t + cam.t)).max() < 1e-15


def test_rig_pose_test_builds_without_a_gpu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    r = subprocess.run([os.path.join(ROOT, "host", "bin", "rig_pose_test")], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
