"""fid_map_save_file (include/fid_abi.h: "building the map") through ctypes, no device: the file fiducial_slam reads as its map_file,
read back by fid_map_load_file to the six printed decimals."""
import numpy as np

import map_build_restatement as mb
from fiducials_amd import _lib
from fiducials_amd.detector import load_map, map_entry_from_rpy, save_map

FIXED, SOLVED, FEW = _lib.BUILD_MARKER_FIXED, _lib.BUILD_MARKER_SOLVED, _lib.BUILD_MARKER_FEW_VIEWS


def _markers():
    """Five records: a fixed one, three solved ones (one at the gimbal lock) and one left out; slots 0 .. 3, links 0 - 1 - 2, 3 alone."""
    rpy = [(0.0, 0.0, 0.0), (12.5, -30.25, 170.0), (-100.0, 60.0, -45.5), (33.0, 90.0, 0.0), (1.0, 2.0, 3.0)]
    xyz = [(0.0, 0.0, 0.0), (1.25, -0.5, 0.125), (-3.0, 2.0, 0.75), (0.1, 0.2, 0.3), (9.0, 9.0, 9.0)]
    m = np.zeros(5, _lib.BUILD_MARKER_DTYPE)
    for k in range(5):
        m["entry"][k] = map_entry_from_rpy(100 - 10 * k, 0.14, xyz[k], rpy[k])
    m["id"] = m["entry"]["id"]
    m["status"] = [FIXED, SOLVED, SOLVED, SOLVED, FEW]
    m["slot"] = [3, 2, 1, 0, -1]  # (ids descend, so the slots -- id order -- do too)
    m["n_views"] = [7, 5, 3, 2, 1]
    link = lambda *slots: sum(1 << s for s in slots)
    m["links"][:, 0] = [link(3, 2), link(3, 2, 1), link(2, 1), link(0), 0]
    for k in (1, 2, 3):
        m["cov"][k] = np.diag([1e-4, 2e-4, 3e-4, 1e-6 * k, 2e-6 * k, 6e-6 * k])
    m["cov"][0] = 0.0
    return m, rpy, xyz


def test_round_trip_with_a_fixed_marker_and_links(tmp_path):
    m, rpy, xyz = _markers()
    path = tmp_path / "map.txt"
    save_map(path, m)
    lines = path.read_text().splitlines()
    assert len(lines) == 4  # the marker that was left out is not written
    f = [ln.split() for ln in lines]
    assert [int(x[0]) for x in f] == [100, 90, 80, 70]
    assert [int(x[8]) for x in f] == [7, 5, 3, 2]
    assert [[int(y) for y in x[9:]] for x in f] == [[90], [80, 100], [90], []]  # ascending, the marker itself left out
    assert float(f[0][7]) == 0.0  # the fixed marker's variance, as the reference's origin
    assert [abs(float(f[k][7]) - 3e-6 * k) < 5e-7 for k in (1, 2, 3)] == [True] * 3  # the mean of the translational variances
    for k in range(4):  # the restatement's line, character for character
        assert lines[k] + "\n" == mb.file_line(int(m["id"][k]), m["entry"]["R"][k], m["entry"]["t"][k], float(f[k][7]), int(m["n_views"][k]), [int(y) for y in f[k][9:]])
    e, skipped = load_map(str(path), 0.14)
    assert skipped == 0 and list(e["id"]) == [100, 90, 80, 70]
    for k in range(4):
        assert np.abs(e["t"][k] - m["entry"]["t"][k]).max() <= 1e-6  # metres
        # every printed angle to 1e-6 degrees (at the gimbal lock, row 3, the file carries yaw 0 and the whole turn about the vertical in roll)
        want = np.array(rpy[k]) if k != 3 else np.array([rpy[k][0] - rpy[k][2], 90.0, 0.0])
        assert np.abs(np.array([float(x) for x in f[k][4:7]]) - want).max() <= 1e-6, (k, f[k][4:7])
        # and the rotation read back: what is left between the two, as an angle (from the skew part, which is exact for small angles)
        dR = e["R"][k] @ m["entry"]["R"][k].T
        angle = np.degrees(np.arcsin(min(1.0, np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2)))
        assert angle <= 1e-6, (k, angle)
        if k != 3:
            assert np.abs(mb.rpy_deg(e["R"][k]) - np.array(rpy[k])).max() <= 1e-6


def test_an_empty_list_writes_an_empty_file(tmp_path):
    path = tmp_path / "empty.txt"
    save_map(path, np.zeros(0, _lib.BUILD_MARKER_DTYPE))
    assert path.read_text() == ""
    e, skipped = load_map(str(path), 0.14)
    assert len(e) == 0 and skipped == 0


def test_refusals(tmp_path):
    L = _lib.load()
    m, _, _ = _markers()
    assert L.fid_map_save_file(None, m.ctypes.data, 5) == _lib.FID_E_INVALID_ARG
    assert L.fid_map_save_file(str(tmp_path / "x").encode(), None, 5) == _lib.FID_E_INVALID_ARG
    assert L.fid_map_save_file(str(tmp_path / "x").encode(), m.ctypes.data, -1) == _lib.FID_E_INVALID_ARG
    assert L.fid_map_save_file(str(tmp_path / "no" / "such" / "dir" / "x").encode(), m.ctypes.data, 5) == _lib.FID_E_INVALID_ARG
    assert b"cannot open" in L.fid_map_last_error()
