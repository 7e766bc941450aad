"""Printable STag markers for every HD library -- the STag counterpart of `marker_gen`.

The reference ships no STag generator ("You can generate STag markers from any library you prefer", stag_detect/README.md),
only 15 raster pages of HD11 markers (stag_detect/test/test.pdf).  Here a marker is drawn as vector primitives straight from
the library's codewords (`stag.load_library`), in marker units where the outer black square is [0, 1]^2 (x right, y down,
corner 0 at the origin: the order of Marker::corners):
  - the black square;
  - the white disc of radius DISC_RADIUS about the centre;
  - one black circle at code point i (Stag::fillCodeLocations, Stag.cpp:129-174; `synth.stag_code_locations`) for each bit i
    of the codeword that is 1 (Stag::readCode thresholds the samples inverted: a dark code point reads 1).
`render` rasterises them (numpy, supersampled), `gen_svg` / `write_pdf` draw them as vectors on a page in the style of
`marker_gen`'s: a white quiet zone, cut marks and measuring lines exactly `side_mm` long, the label "<id> HD<hd>".  `side_mm`
is the printed side of the black square: the length the node's ~marker_size means (the corners sit at +-marker_size / 2,
stag_detect.cpp:144-162), 180 mm = the node's default 0.18 m.

    python -m fiducials_amd.stag_marker_gen 0 20 markers.pdf --hd 11 [--side-mm 180] [--paper-size letter|a4]
    python -m fiducials_amd.stag_marker_gen 0 20 outdir/ --hd 21 --svg
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from .marker_gen import PAPER, pdf_file, pdf_text
from .stag import load_library
from .synth import stag_code_locations

HD_VALUES = (11, 13, 15, 17, 19, 21, 23)
SIDE_MM = 180.0  # the node's default ~marker_size, 0.18 m (stag_detect.cpp:106)
QUIET_MM = 10.0  # white paper between the black square and the cut lines: what is left around the marker once it is cut out
PRINT_MARGIN_MM = 5.0  # no line or label closer to the paper's edge than this (printers leave such a margin blank)
LABEL_DROP_MM = 30.0  # label baseline below the square, as marker_gen's page

# Measured from the reference's printed markers (stag_detect/test/test.pdf, the 15 pages of tests/golden/stag_hd11_pdf.npz),
# each page mapped into marker units with the homography of the four corners the reference's detector returns for it and
# thresholded at its Otsu level.  The disc comes out at Stag's own outerCircleRadius (Stag.cpp:134).  The printed code never
# reaches further than 0.3505 from the centre on any page: a white ring of 0.05 stays inside the disc's edge, and the outer
# ring's black shapes end 0.034 - 0.035 beyond their code points (the largest dark radius along the ray through each point).
# That ring matters to the detector: PoseRefiner fits its ellipse to the disc's edge, and outer circles that come closer to
# it (0.045, the radius that matches most pixels) pull the refined corners of a 72 px marker outward by up to 1.6 % of its
# side.  The inner radius maximises the pixels that agree inside the square (a 2 px band at its edges left out).  The
# printed code shapes are smoothed unions of circles -- black neighbours are joined by fillets, which circles do not draw --
# so 93.4 % of the pixels agree on average; tests/test_stag_marker_gen.py states the per-page figures.
DISC_RADIUS = 0.4
CODE_RADIUS_INNER = 0.063  # code points 0 - 6 of each quadrant (Stag::fillCodeLocations' order)
CODE_RADIUS_OUTER = 0.035  # code points 7 - 11: the ring at 0.31 from the centre, ending 0.35 from it as the printed code


def _codeword(hd: int, marker_id: int) -> int:
    if hd not in HD_VALUES:
        raise ValueError(f"invalid library HD{hd}: possible values are 11, 13, 15, 17, 19, 21 or 23")
    words = load_library(hd)
    n = len(words) // 4  # rotation 0 block first (Decoder::Decoder): ids index it
    if not 0 <= marker_id < n:
        raise ValueError(f"marker id {marker_id} not in library HD{hd} (ids 0 .. {n - 1})")
    return int(words[marker_id])


def marker_primitives(hd: int, marker_id: int):
    """The marker in marker units: (square (x, y, side) black, disc (cx, cy, r) white, [(cx, cy, r) black per code bit 1])."""
    word = _codeword(hd, marker_id)
    locs = stag_code_locations()
    circles = [(float(locs[i, 0]), float(locs[i, 1]), CODE_RADIUS_INNER if i % 12 < 7 else CODE_RADIUS_OUTER)
               for i in range(48) if (word >> i) & 1]
    return (0.0, 0.0, 1.0), (0.5, 0.5, DISC_RADIUS), circles


def render(hd: int, marker_id: int, px: int, quiet_zone: float = 0.125, ss: int = 4) -> np.ndarray:
    """The marker as a uint8 image (0 black, 255 white): `px` pixels across the black square, a white quiet zone of
    round(quiet_zone * px) pixels around it (0.125: the reference's pages, an 800 px square on 1000 x 1000), each pixel the mean
    of ss x ss samples.  Pixel (r, c) covers marker coordinates [(c - q) / px, (c + 1 - q) / px) x [(r - q) / px, ...)."""
    square, disc, circles = marker_primitives(hd, marker_id)
    q = int(round(quiet_zone * px))
    n = px + 2 * q
    t = ((np.arange(n * ss) + 0.5) / ss - q) / px  # sample positions in marker units, the same on both axes
    white = np.ones((n * ss, n * ss), bool)

    def span(a, b):  # the samples in [a, b)
        return slice(*np.searchsorted(t, [a, b]))

    x, y, s = square
    white[span(y, y + s), span(x, x + s)] = False
    for (cx, cy, r), value in [(disc, True)] + [(c, False) for c in circles]:
        rows, cols = span(cy - r, cy + r), span(cx - r, cx + r)
        white[rows, cols][(t[rows, None] - cy) ** 2 + (t[None, cols] - cx) ** 2 < r * r] = value
    cover = white.reshape(n, ss, n, ss).mean(axis=(1, 3))
    return np.rint(cover * 255).astype(np.uint8)


def max_side_mm(paper_size) -> float:
    """The largest black square a page of `paper_size` holds with its quiet zone, cut marks and label inside the margins."""
    pw, ph = paper_size
    return min(pw - 2 * (QUIET_MM + PRINT_MARGIN_MM), ph - 2 * (LABEL_DROP_MM + PRINT_MARGIN_MM))


def page_layout(hd: int, marker_id: int, side_mm: float, paper_size):
    """The page as drawing primitives in millimetres (origin top left, painted in this order): the black square (x, y, side),
    circles (cx, cy, r, white?), hair lines, texts (x, baseline y, pt, string)."""
    if not 0 < side_mm <= max_side_mm(paper_size):
        raise ValueError(f"side_mm {side_mm:g} does not fit the page: a {paper_size[0]:g} x {paper_size[1]:g} mm sheet holds a "
                         f"square of up to {max_side_mm(paper_size):g} mm with its {QUIET_MM:g} mm quiet zone and its label")
    _, (dx, dy, dr), code = marker_primitives(hd, marker_id)
    pw, ph = paper_size
    s = side_mm
    x0, y0 = (pw - s) / 2, (ph - s) / 2
    square = (x0, y0, s)
    circles = [(x0 + dx * s, y0 + dy * s, dr * s, True)] + [(x0 + cx * s, y0 + cy * s, r * s, False) for cx, cy, r in code]
    lines = []
    for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):  # cut marks at the four corners of the quiet zone
        cx = pw / 2 + sx * (s / 2 + QUIET_MM)
        cy = ph / 2 + sy * (s / 2 + QUIET_MM)
        lines.append((cx, cy, cx - sx * 2, cy))
        lines.append((cx, cy, cx, cy - sy * 2))
    top, bottom = ph / 2 - s / 2 - QUIET_MM, ph / 2 + s / 2 + QUIET_MM
    left, right = pw / 2 - s / 2 - QUIET_MM, pw / 2 + s / 2 + QUIET_MM
    for yy in (top, bottom):  # measuring lines along the cut: exactly side_mm long
        lines.append((x0, yy, x0 + s, yy))
    for xx in (left, right):
        lines.append((xx, y0, xx, y0 + s))
    texts = [(pw / 2, top - 1, 8, "This line should be exactly %gcm long." % (s / 10)),
             (pw / 2, (ph + s) / 2 + LABEL_DROP_MM, 24, "%d HD%d" % (marker_id, hd))]
    return square, circles, lines, texts


def gen_svg(marker_id: int, *, hd: int, side_mm: float = SIDE_MM, paper_size=PAPER["letter"]) -> str:
    square, circles, lines, texts = page_layout(hd, marker_id, side_mm, paper_size)
    pw, ph = paper_size
    x, y, s = square
    out = ['<svg width="%gmm" height="%gmm" viewBox="0 0 %g %g" version="1.1" xmlns="http://www.w3.org/2000/svg">' % (pw, ph, pw, ph),
           '  <rect x="%.4f" y="%.4f" width="%.4f" height="%.4f" style="stroke:none; fill:black"/>' % (x, y, s, s)]
    for cx, cy, r, white in circles:
        out.append('  <circle%s cx="%.4f" cy="%.4f" r="%.4f" style="stroke:none; fill:%s"/>'
                   % ("" if white else ' class="code"', cx, cy, r, "white" if white else "black"))
    for x1, y1, x2, y2 in lines:
        out.append('  <line x1="%.4f" y1="%.4f" x2="%.4f" y2="%.4f" style="stroke:black; stroke-width:0.2"/>' % (x1, y1, x2, y2))
    for x, y, size, s in texts:
        out.append('  <text x="%.4f" y="%.4f" text-anchor="middle" style="font-family:arial; font-size:%gpt;">%s</text>' % (x, y, size * 25.4 / 72 * 0.75, s))
    out.append("</svg>")
    return "\n".join(out) + "\n"


KAPPA = 0.5522847498307936  # a quarter circle as one cubic Bezier: control points at kappa * r along the tangents


def write_pdf(path: str, marker_ids, *, hd: int, side_mm: float = SIDE_MM, paper_size=PAPER["letter"]) -> None:
    """One marker per page, vector graphics (circles as four Bezier quarters), built-in Helvetica."""
    pages = [page_layout(hd, mid, side_mm, paper_size) for mid in marker_ids]  # every id and the side checked before writing
    k = 72 / 25.4  # mm -> pt
    ph = paper_size[1]
    streams = []
    for square, circles, lines, texts in pages:
        x, y, s = square
        c = ["0 g", "%.3f %.3f %.3f %.3f re f" % (x * k, (ph - y - s) * k, s * k, s * k)]
        for cx, cy, r, white in circles:
            X, Y, R = cx * k, (ph - cy) * k, r * k
            a = KAPPA * R
            c.append("%d g %.3f %.3f m" % (white, X + R, Y))
            c.append("%.3f %.3f %.3f %.3f %.3f %.3f c" % (X + R, Y + a, X + a, Y + R, X, Y + R))
            c.append("%.3f %.3f %.3f %.3f %.3f %.3f c" % (X - a, Y + R, X - R, Y + a, X - R, Y))
            c.append("%.3f %.3f %.3f %.3f %.3f %.3f c" % (X - R, Y - a, X - a, Y - R, X, Y - R))
            c.append("%.3f %.3f %.3f %.3f %.3f %.3f c f" % (X + a, Y - R, X + R, Y - a, X + R, Y))
        c.append("0 G 0.5 w")
        for x1, y1, x2, y2 in lines:
            c.append("%.3f %.3f m %.3f %.3f l S" % (x1 * k, (ph - y1) * k, x2 * k, (ph - y2) * k))
        c.append("0 g")
        for x, y, size, s in texts:
            c.append(pdf_text(x, y, size, s, ph))
        streams.append("\n".join(c).encode("ascii"))
    with open(path, "wb") as fh:
        fh.write(pdf_file(streams, paper_size))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Generate STag markers.")
    ap.add_argument("startId", type=int, help="start of marker range to generate")
    ap.add_argument("endId", type=int, help="end of marker range to generate")
    ap.add_argument("out", type=str, help="PDF file to store the markers in (or a directory with --svg)")
    ap.add_argument("--hd", type=int, required=True, choices=HD_VALUES, help="marker library: the node's libraryHD")
    ap.add_argument("--side-mm", dest="side_mm", type=float, default=SIDE_MM,
                    help="printed side of the black square in mm: 1000 x the node's ~marker_size (default %(default)g)")
    ap.add_argument("--paper-size", dest="paper_size", default="letter", choices=sorted(PAPER), help="paper size to use (letter or a4)")
    ap.add_argument("--svg", action="store_true", help="one self-contained SVG per marker into the directory `out`")
    a = ap.parse_args(argv)
    ids = list(range(a.startId, a.endId + 1))
    paper = PAPER[a.paper_size]
    if a.svg:
        svgs = [gen_svg(i, hd=a.hd, side_mm=a.side_mm, paper_size=paper) for i in ids]  # every id checked before a file is written
        os.makedirs(a.out, exist_ok=True)
        for i, svg in zip(ids, svgs):
            with open(os.path.join(a.out, "marker%d.svg" % i), "w") as fh:
                fh.write(svg)
    else:
        write_pdf(a.out, ids, hd=a.hd, side_mm=a.side_mm, paper_size=paper)
    print("After printing, please make sure that the long lines around the marker are EXACTLY %gcm long, and run stag_detect "
          "with libraryHD %d and marker_size %g." % (a.side_mm / 10, a.hd, a.side_mm / 1000))
    return 0


if __name__ == "__main__":
    sys.exit(main())
