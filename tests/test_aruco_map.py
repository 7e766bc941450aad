"""The map of fiducials on the host (fid_map_load_file, fid_map_entry_from_rpy, load_map): the file fiducial_slam keeps, read
against literals; and the board generator's scenes as the CPU oracle's detector sees them.  No device."""
import ctypes as C

import numpy as np
import pytest

import aruco_map_cases as mc
from fiducials_amd import _lib
from fiducials_amd.detector import MAP_ENTRY_DTYPE, MAP_POSE_DTYPE, FidError, load_map, map_entry_from_rpy
from fiducials_amd.dictionary import get_predefined_dictionary


def _rz_ry_rx(roll, pitch, yaw):
    """Rz(yaw) Ry(pitch) Rx(roll) written out, angles in degrees (tf2::Quaternion::setRPY)."""
    r, p, y = np.deg2rad([roll, pitch, yaw])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def test_struct_mirrors_have_the_headers_sizes():
    assert C.sizeof(_lib.FidMapEntry) == MAP_ENTRY_DTYPE.itemsize == 8 + 8 + 72 + 24
    assert C.sizeof(_lib.FidMapPoseOut) == MAP_POSE_DTYPE.itemsize == 8 + 8 * (3 + 3 + 9 + 9 + 3 + 1)


def test_the_reference_fixture_line_is_the_identity(tmp_path):
    p = tmp_path / "map.txt"
    p.write_text("111 0 0 0 0 0 0 0 0\n")
    e, skipped = load_map(str(p), 0.14)
    assert skipped == 0 and e["id"].tolist() == [111] and e["len"].tolist() == [0.14]
    assert np.array_equal(e["R"][0], np.eye(3)) and np.array_equal(e["t"][0], np.zeros(3))


def test_angles_links_short_lines_and_overrides(tmp_path):
    p = tmp_path / "map.txt"
    p.write_text("7 1.5 -2.25 0.5 10 20 30 0.001 12\n"
                 "8 0.1 0.2 0.3 -170.5 45.25 95 0.02 3 7 111 245\n"   # with links
                 "9 0.1 0.2 0.3\n"                                     # short: passed over
                 "not a line\n"
                 "\n"
                 "245 -1 0 2 0 0 90 0.5 1")                             # no newline at the end of the file
    e, skipped = load_map(str(p), 0.14, {8: 0.2, 99: 0.3})
    assert skipped == 3 and e["id"].tolist() == [7, 8, 245]
    assert e["len"].tolist() == [0.14, 0.2, 0.14]
    assert np.abs(e["R"][0] - _rz_ry_rx(10, 20, 30)).max() < 1e-15 and e["t"][0].tolist() == [1.5, -2.25, 0.5]
    assert np.abs(e["R"][1] - _rz_ry_rx(-170.5, 45.25, 95)).max() < 1e-15 and e["t"][1].tolist() == [0.1, 0.2, 0.3]
    assert np.abs(e["R"][2] - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])).max() < 1e-15
    for k, (fid, xyz, rpy) in enumerate(((7, (1.5, -2.25, 0.5), (10, 20, 30)), (8, (0.1, 0.2, 0.3), (-170.5, 45.25, 95)), (245, (-1, 0, 2), (0, 0, 90)))):
        b = map_entry_from_rpy(fid, float(e["len"][k]), xyz, rpy)
        assert b.tobytes() == e[k].tobytes()


def test_what_the_loader_refuses(tmp_path):
    L = _lib.load()
    with pytest.raises(FidError) as ex:
        load_map(str(tmp_path / "nowhere.txt"), 0.14)
    assert ex.value.status == _lib.FID_E_INVALID_ARG and "nowhere.txt" in str(ex.value)
    p = tmp_path / "twice.txt"
    p.write_text("5 0 0 0 0 0 0 0 0\n6 1 0 0 0 0 0 0 0\n5 2 0 0 0 0 0 0 0\n")
    with pytest.raises(FidError) as ex:
        load_map(str(p), 0.14)
    assert ex.value.status == _lib.FID_E_INVALID_ARG and "5" in str(ex.value) and "twice" in str(ex.value)
    # more entries than the caller has room for: the count comes back
    q = tmp_path / "three.txt"
    q.write_text("".join(f"{i} {i} 0 0 0 0 0 0 0\n" for i in range(3)))
    buf = np.zeros(2, MAP_ENTRY_DTYPE)
    n, sk = C.c_int32(0), C.c_int32(0)
    assert L.fid_map_load_file(str(q).encode(), 0.14, buf.ctypes.data, 2, C.byref(n), C.byref(sk)) == _lib.FID_E_CAPACITY
    assert n.value == 3 and b"3" in L.fid_map_last_error()
    assert L.fid_map_load_file(str(q).encode(), 0.0, buf.ctypes.data, 2, C.byref(n), C.byref(sk)) == _lib.FID_E_INVALID_ARG
    with pytest.raises(FidError):
        map_entry_from_rpy(1, 0.0, (0, 0, 0), (0, 0, 0))


def test_board_scenes_show_every_marker_where_the_map_puts_it():
    """make_aruco_board_frame: the CPU oracle's detector finds every marker of a scene, its corners within two pixels of the map's
    corners projected through the rendering pose (the two-wall corner is seen at 45 degrees); an occluded marker is missing."""
    import oracle
    d = get_predefined_dictionary(mc.DICT)
    for name, pose in (("3x2", 1), ("corner", 0)):
        fr = mc.scene(name, pose)
        assert np.abs(mc.project(fr.corners_map.reshape(-1, 3), fr.R, fr.tvec, mc.K, np.zeros(5)).reshape(-1, 4, 2) - fr.corners_image).max() < 1e-9
        ids, corners = oracle.detect(fr.image, d)
        assert sorted(ids.tolist()) == fr.ids.tolist()
        for i, c in zip(ids, corners):
            assert np.abs(c - fr.corners_image[fr.ids.tolist().index(int(i))]).max() < 2.0
    ids, _ = oracle.detect(mc.scene("3x2", 1, without=2).image, d)
    assert sorted(ids.tolist()) == [20, 21, 23, 24, 25]
