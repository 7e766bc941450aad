"""The printable ChArUco sheet (fiducials_amd.marker_gen) against the board's object points and the synthetic frame: sheet, pose tables
and picture describe the same board."""
import re

import numpy as np

import charuco_cases as cc
from fiducials_amd import marker_gen, synth
from fiducials_amd.dictionary import draw_marker


def _rects(svg):
    out = []
    for m in re.finditer(r'<rect (class="cell" )?x="([-0-9.]+)" y="([-0-9.]+)" width="([-0-9.]+)" height="([-0-9.]+)" style="stroke:none; fill:(\w+)"', svg):
        out.append((m.group(6), *[float(m.group(i)) for i in (2, 3, 4, 5)]))
    return out


def test_the_sheet_is_drawn_from_the_object_points(tmp_path):
    b, d = cc.board("5x4"), cc.dictionary()
    pw, ph = marker_gen.PAPER["a4"]
    rects = _rects(marker_gen.gen_charuco_svg(b, cc.DICT, marker_gen.PAPER["a4"]))
    black = [r for r in rects if r[0] == "black"]
    x0, y0, bh = (pw - 200.0) / 2, (ph - 160.0) / 2, 160.0
    squares = [r for r in black if abs(r[3] - 40.0) < 1e-6]
    assert len(squares) == 10 and len(black) == 20
    assert any(abs(r[1] - x0) < 1e-3 and abs(r[2] - (y0 + bh - 40.0)) < 1e-3 for r in squares)  # square (0, 0): bottom left of the board
    for k in range(b.n_markers):  # every marker's square sits where its object points are
        c0 = b.marker_object_points[k, 0]
        assert any(abs(r[1] - (x0 + c0[0] * 1000)) < 1e-3 and abs(r[2] - (y0 + bh - c0[1] * 1000)) < 1e-3 and abs(r[3] - 24.0) < 1e-3 for r in black)
    ncell = d.marker_size + 2
    n_white = sum(int((draw_marker(d, int(i), ncell, 1) > 0).sum()) for i in b.ids)
    assert len([r for r in rects if r[0] == "white"]) == n_white
    marker_gen.write_charuco_pdf(str(tmp_path / "board.pdf"), b, cc.DICT, marker_gen.PAPER["a4"])
    data = (tmp_path / "board.pdf").read_bytes()
    assert data.startswith(b"%PDF-1.4") and data.count(b" re f") == len(rects)
    assert marker_gen.main(["0", "0", str(tmp_path / "cli.pdf"), str(cc.DICT), "--charuco", "5x4:40:24", "--paper-size", "a4"]) == 0
    assert (tmp_path / "cli.pdf").read_bytes() == data
    try:
        marker_gen.gen_charuco_svg(cc.board("22x23"), cc.DICT, allow_fillers=True)
        raise AssertionError("a board larger than the page must be refused")
    except ValueError as e:
        assert "does not fit" in str(e)


def test_the_picture_shows_the_sheet():
    """Frontal and close: the rendered frame, sampled at the projections of the sheet's white and black cells, shows white and black."""
    b, d = cc.board("5x4"), cc.dictionary()
    R, t = cc.board_pose("5x4", (0.0, 0.0, 0.0), 0.30)
    fr = synth.make_charuco_frame(d, b, cc.K, R, t, seed=1, width=cc.W, height=cc.H, noise_sigma=0.0)
    black, white = b.layout(d)
    squares, marker_rects = black[:10], black[10:]

    def level(r):
        x, y, w, h = r
        P = np.array([[x + w / 2, y + h / 2, 0.0]]) @ R.T + t
        u, v = cc.K[0, 0] * P[0, 0] / P[0, 2] + cc.K[0, 2], cc.K[1, 1] * P[0, 1] / P[0, 2] + cc.K[1, 2]
        return float(fr.image[int(round(v)), int(round(u))])

    assert all(level(r) < 60 for r in squares) and all(level(r) > 190 for r in white)
    assert all(level((x + 0.0005, y + 0.0005, 0.002, 0.002)) < 60 for x, y, w, h in marker_rects)  # a marker's border cell
    assert fr.markers_image.shape == (10, 4, 2) and fr.corners_image.shape == (12, 2)
