"""ChArUco boards on the CPU: the board's tables against an enumeration written by hand, fiducials_amd.charuco against the restatement,
and the whole chain restated -- oracle.detect, the 4-point homographies, the windows, oracle.corner_subpix -- on rendered boards against
the true projections.  No device."""
import numpy as np
import pytest

import charuco_cases as cc
import charuco_restatement as cr
from fiducials_amd import _lib
from fiducials_amd.charuco import CharucoBoard


def test_the_abi_names_the_entry_points():
    for name in ("fid_set_charuco_board", "fid_charuco_last_cam", "fid_charuco_interpolate_cam", "fid_charuco_pose_last_cam", "fid_charuco_pose_cam"):
        assert name in _lib.SYMBOLS
    assert _lib.CHARUCO_CORNER_DTYPE.itemsize == 24 and _lib.CHARUCO_POSE_DTYPE.itemsize == 8 + 8 * (3 + 3 + 9 + 9 + 3 + 1)


def test_a_3x3_board_against_the_enumeration():
    """3 x 3 squares of 0.5 with markers of 0.25 (all exact in float), first id 7.  White squares in marker order: (1, 0), (0, 1),
    (2, 1), (1, 2)."""
    b = cr.Board(3, 3, 0.5, 0.25, 7)
    assert b.ids.tolist() == [7, 8, 9, 10] and b.n_corners == 4
    # marker 0 sits in square (1, 0): d = 0.125, corner 0 = (0.625, 0.375), then clockwise seen from the front
    assert b.marker_obj[0].tolist() == [[0.625, 0.375, 0], [0.875, 0.375, 0], [0.875, 0.125, 0], [0.625, 0.125, 0]]
    assert b.marker_obj[1].tolist() == [[0.125, 0.875, 0], [0.375, 0.875, 0], [0.375, 0.625, 0], [0.125, 0.625, 0]]  # square (0, 1)
    assert b.marker_obj[2, 0].tolist() == [1.125, 0.875, 0] and b.marker_obj[3, 0].tolist() == [0.625, 1.375, 0]      # (2, 1), (1, 2)
    assert b.corner_obj.tolist() == [[0.5, 0.5, 0], [1.0, 0.5, 0], [0.5, 1.0, 0], [1.0, 1.0, 0]]
    # corner 0 (cx + cy even): squares (1, 0) and (0, 1) -> markers 0, 1; of marker 0 its bottom-left... the corner nearest (0.5, 0.5)
    assert b.near_marker.tolist() == [[0, 1], [0, 2], [1, 3], [2, 3]]
    assert b.near_corner.tolist() == [[0, 2], [1, 3], [1, 3], [0, 2]]
    # the package's board is the same board
    p = CharucoBoard(3, 3, 0.5, 0.25, 7)
    assert np.array_equal(p.marker_object_points, b.marker_obj) and np.array_equal(p.corner_object_points, b.corner_obj)
    assert np.array_equal(p.nearest_markers, b.near_marker) and np.array_equal(p.nearest_corners, b.near_corner)
    assert p.ids.tolist() == b.ids.tolist()


@pytest.mark.parametrize("name", sorted(cc.BOARDS))
def test_the_package_board_is_the_restated_board(name):
    p, b = cc.board(name), cc.rboard(name)
    assert p.n_markers == b.n_markers == p.squares_x * p.squares_y // 2 and p.n_corners == b.n_corners
    assert np.array_equal(p.marker_object_points, b.marker_obj) and np.array_equal(p.corner_object_points, b.corner_obj)
    assert np.array_equal(p.nearest_markers, b.near_marker) and np.array_equal(p.nearest_corners, b.near_corner)
    # every nearest marker corner lies (s - m) / 2 from the chessboard corner on both axes
    d = (p.square_len - p.marker_len) / 2
    for i in range(p.n_corners):
        for k, c in zip(p.nearest_markers[i], p.nearest_corners[i]):
            assert np.allclose(np.abs(p.marker_object_points[k, c, :2] - p.corner_object_points[i, :2]), d, rtol=0, atol=1e-7)


def test_the_board_as_a_map_and_as_a_raster():
    p = cc.board("5x4_dyadic")
    e = p.as_map_entries()
    h = float(np.float32(p.marker_len / 2))
    rebuilt = np.array([[-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0]])[None] + e["t"][:, None, :]
    assert np.array_equal(rebuilt, p.marker_object_points) and e["id"].tolist() == p.ids.tolist()
    img = cc.board("5x4").draw(cc.dictionary(), 40)
    assert img.shape == (160, 200) and img[159, 0] == 0 and img[159, 40] == 255 and img[0, 0] == 255  # squares (0, 0), (1, 0), (0, 3)
    assert img[159 - 8, 48] == 0 and img[159 - 4, 44] == 255  # marker 0's black border starts 8 px inside its white square
    black, white = cc.board("5x4").layout(cc.dictionary())
    assert len(black) == 10 + 10 and all(w > 0 and hh > 0 for _, _, w, hh in black + white)


def test_duplicates_foreign_ids_and_lost_markers_in_the_gather():
    b = cc.rboard("5x4_id40")
    assert cr.gather(b, [40, 41, 41, 3, 49, 50, 45]) == {0: 0, 9: 4, 5: 6}
    assert cr.pose_status(b, [0, 1, 2]) == cr.POSE_FEW and cr.pose_status(b, [0, 1, 2, 3]) == cr.POSE_COLLINEAR
    assert cr.pose_status(b, [0, 5, 10, 1]) == cr.POSE_OK and cr.pose_status(b, [0, 5, 10, 0]) == cr.POSE_COLLINEAR  # 4 x 3 corners a row


@pytest.mark.parametrize("name,min_found", [("frontal", 10), ("tilted", 9)])
def test_rendered_boards_end_to_end_against_the_truth(name, min_found):
    """5 x 4 board, 640 x 480, square 0.04, marker 0.024.  A wrongly numbered corner is off by a whole square, so a quarter of the
    smallest projected square side is a condition on every refined corner, not a measurement."""
    import oracle
    b, fr = cc.rboard("5x4"), cc.view(name)
    ids, corners = oracle.detect(fr.image, cc.dictionary())
    found = len(cr.gather(b, ids))
    print(name, "markers found", found, "of", b.n_markers)
    assert found >= min_found and found >= 9
    for min_markers in (2, 1):
        kept, pos, wins = cr.interpolate(b, ids, corners, cc.W, cc.H, min_markers)
        assert len(kept) >= (10 if min_markers == 2 else 12)
        refined = cr.refine(fr.image, pos, wins)
        truth = fr.corners_image[kept]
        grid = fr.corners_image.reshape(b.squares_y - 1, b.squares_x - 1, 2)
        side = min(np.linalg.norm(np.diff(grid, axis=0), axis=2).min(), np.linalg.norm(np.diff(grid, axis=1), axis=2).min())
        e0, e1 = np.linalg.norm(pos - truth, axis=1), np.linalg.norm(refined - truth, axis=1)
        print(name, "min_markers", min_markers, "corners", len(kept), "windows", wins.min(), "..", wins.max(), "smallest square side %.1f px" % side,
              "interpolated: worst %.3f px" % e0.max(), "refined: worst %.3f px" % e1.max())
        assert e1.max() < side / 4 and e0.max() < side / 4
        assert e1.max() < e0.max()  # the refinement is the point of the board
        r, t = cr.pose(b, cc.K, np.zeros(5), kept, refined)
        assert np.abs(cc.synth._rodrigues(r) - fr.R).max() < 0.02 and np.abs(t - fr.tvec).max() < 0.005
