"""The printable diamond sheet (fiducials_amd.marker_gen --diamond), CharucoDiamond.draw() and the synthetic frame
(synth.make_diamond_frame) against the diamond's own object points: sheet, raster, picture and pose tables describe the same diamond."""
import numpy as np

import diamond_cases as dc
from fiducials_amd import marker_gen, synth
from fiducials_amd.charuco import CharucoDiamond
from fiducials_amd.dictionary import draw_marker
from test_charuco_sheet import _rects

PRINTABLE = (0, 1, 1, 2)  # (ids whose codewords in the shipped table are OpenCV's; a diamond may repeat one)


def test_the_sheet_is_drawn_from_the_object_points(tmp_path):
    b, d = CharucoDiamond(PRINTABLE, 0.04, 0.024), dc.dictionary()
    pw, ph = marker_gen.PAPER["a4"]
    svg = marker_gen.gen_charuco_svg(b, dc.DICT, marker_gen.PAPER["a4"])
    rects = _rects(svg)
    black = [r for r in rects if r[0] == "black"]
    x0, y0, bh = (pw - 120.0) / 2, (ph - 120.0) / 2, 120.0
    squares = [r for r in black if abs(r[3] - 40.0) < 1e-6]
    assert len(squares) == 5 and len(black) == 9  # the four corner squares and the middle one; four marker squares
    assert any(abs(r[1] - (x0 + 40.0)) < 1e-3 and abs(r[2] - (y0 + 40.0)) < 1e-3 for r in squares)  # the middle square is black
    for k in range(4):  # every marker's square sits where its object points are
        c0 = b.marker_object_points[k, 0]
        assert any(abs(r[1] - (x0 + c0[0] * 1000)) < 1e-3 and abs(r[2] - (y0 + bh - c0[1] * 1000)) < 1e-3 and abs(r[3] - 24.0) < 1e-3 for r in black)
    ncell = d.marker_size + 2
    assert len([r for r in rects if r[0] == "white"]) == sum(int((draw_marker(d, int(i), ncell, 1) > 0).sum()) for i in b.ids)
    assert "ChArUco diamond 0,1,1,2, square 40.00 mm, marker 24.00 mm" in svg
    marker_gen.write_charuco_pdf(str(tmp_path / "diamond.pdf"), b, dc.DICT, marker_gen.PAPER["a4"])
    data = (tmp_path / "diamond.pdf").read_bytes()
    assert data.startswith(b"%PDF-1.4") and data.count(b" re f") == len(rects)
    assert marker_gen.main(["0", "0", str(tmp_path / "cli.pdf"), str(dc.DICT), "--diamond", "0,1,1,2", "--paper-size", "a4"]) == 0
    assert (tmp_path / "cli.pdf").read_bytes() == data
    assert marker_gen.main(["0", "0", str(tmp_path / "svg"), str(dc.DICT), "--diamond", "0,1,1,2:50:30", "--svg"]) == 0
    assert "square 50.00 mm, marker 30.00 mm" in (tmp_path / "svg" / "diamond0_1_1_2.svg").read_text()
    for bad in ((0, 1, 2), (0, 1, 2, -3)):
        try:
            CharucoDiamond(bad, 0.04, 0.024)
            raise AssertionError("a diamond has four ids")
        except ValueError:
            pass


def test_the_raster_is_drawn_from_the_object_points():
    b, d = CharucoDiamond(PRINTABLE, 0.04, 0.024), dc.dictionary()
    img = b.draw(d, 40)
    assert img.shape == (120, 120)
    assert img[119, 0] == 0 and img[60, 60] == 0 and img[0, 119] == 0 and img[119, 60] == 255  # squares (0, 0), (1, 1), (2, 2) black; (1, 0) white
    # marker 0 (square (1, 0), the bottom middle one) covers its object points' pixels: 8 px inside its square, 24 px wide
    assert np.array_equal(img[120 - 32:120 - 8, 48:72], draw_marker(d, 0, 24, 1))
    assert np.array_equal(img[8:32, 48:72], draw_marker(d, 2, 24, 1))  # marker 3, square (1, 2), carries the fourth id
    assert np.array_equal(img[48:72, 8:32], img[48:72, 88:112])        # markers 1 and 2 carry the same id


def test_the_picture_shows_the_sheet():
    """A diamond and a loose marker, frontal and close: the rendered frame, sampled at the projections of the sheet's white and black
    cells, shows white and black; the true projections it returns are those of the object points."""
    b, d = dc.diamond(dc.ONE_IDS), dc.dictionary()
    R, t = dc.diamond_pose((0.0, 0.0, 0.0), 0.27, shift_px=(-60.0, 0.0))
    Rl, tl = dc.loose_pose(dc.MARKER, (0.0, 0.0, 0.0), 0.27, 0.0, (200.0, 0.0))
    fr = synth.make_diamond_frame(d, [(b, R, t)], dc.K, seed=1, loose=[(44, dc.MARKER, Rl, tl)], width=dc.W, height=dc.H, noise_sigma=0.0)
    black, white = b.layout(d)
    squares, marker_rects = black[:5], black[5:]

    def level(r, Rr=R, tr=t):
        x, y, w, h = r
        u, v = dc.project(np.array([[x + w / 2, y + h / 2, 0.0]]), Rr, tr, dc.K, dc.Z5)[0]
        return float(fr.image[int(round(v)), int(round(u))])

    assert all(level(r) < 60 for r in squares) and all(level(r) > 190 for r in white)
    assert all(level((x + 0.0005, y + 0.0005, 0.002, 0.002)) < 60 for x, y, w, h in marker_rects)  # a marker's border cell
    assert fr.markers_image.shape == (1, 4, 4, 2) and fr.corners_image.shape == (1, 4, 2) and fr.loose_image.shape == (1, 4, 2)
    assert np.allclose(fr.corners_image[0], dc.project(b.record_object_points, R, t, dc.K, dc.Z5))
    assert np.allclose(fr.corners_image[0], dc.true_corners(R, t))
    assert np.allclose(fr.loose_image[0], dc.hand_loose(dc.MARKER, Rl, tl), atol=1e-3) and fr.loose_ids.tolist() == [44]
    # the loose marker: a black border cell inside its corners, white paper outside them
    lo = synth._LooseMarker(44, dc.MARKER).marker_object_points[0]
    assert level((lo[3, 0] + 0.0005, lo[3, 1] + 0.0005, 0.002, 0.002), Rl, tl) < 60 and level((lo[3, 0] - 0.004, lo[3, 1] - 0.004, 0.002, 0.002), Rl, tl) > 190
    # in the image the record's corners run top left, top right, bottom right, bottom left
    c = fr.corners_image[0]
    assert c[0, 0] < c[1, 0] and c[0, 1] < c[3, 1] and c[2, 0] > c[3, 0] and c[2, 1] > c[1, 1]
