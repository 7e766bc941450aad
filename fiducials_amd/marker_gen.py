"""Printable fiducial markers without cv2 / cairosvg / pdfunite -- the marker-generation row of the reference
(aruco_detect/scripts/create_markers.py:39-54, marker_generation/marker_gen.py:31-98).

The reference rasterises `aruco.drawMarker(dict, id, 2000)` to a PNG, embeds it in an SVG page template (140 mm marker, 4 mm
frame bars, cut marks 14 mm outside the corners, two measuring lines "should be exactly 14.0cm long", the label "<id> D<dicno>")
and converts / concatenates with cairosvg + pdfunite.  Here the page is the same template, but the marker is drawn as vector
cells straight from the dictionary bits (`Dictionary::drawMarker` semantics: (n + 2)^2 cells, one-cell black border, bit 1 =
white), as a self-contained SVG (`gen_svg`) or as one page of a multi-page vector PDF written directly (`write_pdf`).

    python -m fiducials_amd.marker_gen 100 112 markers.pdf [dictionary=7] [--paper-size letter|a4]
    python -m fiducials_amd.marker_gen 100 112 outdir/ --svg
    python -m fiducials_amd.marker_gen 0 0 board.pdf --charuco 5x4:40:24     (a ChArUco board, markers 0 .. 9)
    python -m fiducials_amd.marker_gen 0 0 diamond.pdf --diamond 0,1,1,2  (a ChArUco diamond of those four markers)
"""
from __future__ import annotations

import argparse
import os
import sys

from .dictionary import Dictionary, get_predefined_dictionary

FID_LEN_MM = 140.0  # marker_gen.py:84 ("fid_len": 140.0): the printed marker is 14 cm, the node's default ~fiducial_len
PAPER = {"letter": (215.9, 279.4), "a4": (210.0, 297.0)}  # create_markers.py:41-44


def marker_cells(d: Dictionary, marker_id: int):
    """(n + 2) x (n + 2) matrix of 0 (black) / 1 (white): the cells of `Dictionary::drawMarker` with one border cell."""
    n = d.marker_size
    bits = d.bits(marker_id)
    cells = [[0] * (n + 2) for _ in range(n + 2)]
    for r in range(n):
        for c in range(n):
            cells[r + 1][c + 1] = int(bits[r, c])
    return cells


def page_layout(d: Dictionary, marker_id: int, paper_size):
    """The page as drawing primitives in millimetres (origin top left): black rects, white rects, hair lines, texts."""
    pw, ph = paper_size
    fl = FID_LEN_MM
    x0, y0 = (pw - fl) / 2, (ph - fl) / 2
    cells = marker_cells(d, marker_id)
    nc = len(cells)
    cs = fl / nc
    black = [(x0, y0, fl, fl)]  # the whole marker square, then the white cells on top
    white = [(x0 + c * cs, y0 + r * cs, cs, cs) for r in range(nc) for c in range(nc) if cells[r][c]]
    # the four 4 mm frame bars of the template (inside the marker's own black border)
    black += [(x0, y0, fl, 4.0), (x0, y0 + fl - 4.0, fl, 4.0), (x0, y0, 4.0, fl), (x0 + fl - 4.0, y0, 4.0, fl)]
    cut = max(fl / 10 * 1.4, 10)
    lines = []
    for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):  # cut marks at the four corners
        cx = pw / 2 + sx * (fl / 2 + cut)
        cy = ph / 2 + sy * (fl / 2 + cut)
        lines.append((cx, cy, cx - sx * 2, cy))
        lines.append((cx, cy, cx, cy - sy * 2))
    top, bottom = ph / 2 - fl / 2 - cut, ph / 2 + fl / 2 + cut
    left, right = pw / 2 - fl / 2 - cut, pw / 2 + fl / 2 + cut
    for yy in (top, bottom):  # measuring lines: exactly fid_len long
        lines.append((pw / 2 - fl / 2, yy, pw / 2 + fl / 2, yy))
    for xx in (left, right):
        lines.append((xx, ph / 2 - fl / 2, xx, ph / 2 + fl / 2))
    texts = [(pw / 2, top - 1, 8, "This line should be exactly %scm long." % (fl / 10)),
             (pw / 2, (ph + fl) / 2 + 30, 24, "%d D%d" % (marker_id, _dicno_of(d)))]
    return black, white, lines, texts


def _dicno_of(d: Dictionary) -> int:
    from .dictionary import PREDEFINED

    return PREDEFINED[d.name][0]


def _check_printable(d: Dictionary, marker_id: int, allow_fillers: bool) -> None:
    """A printed marker must interoperate with OpenCV-based detectors: ids whose codeword in the shipped table is a locally
    generated filler (Dictionary.pinned False) are refused unless the caller asks for them explicitly."""
    if not 0 <= marker_id < d.n_markers:
        raise ValueError(f"marker id {marker_id} not in {d.name}")
    if not d.pinned[marker_id] and not allow_fillers:
        raise ValueError(f"marker {marker_id} of {d.name}: the shipped table holds a locally generated filler codeword for this id, "
                         "not OpenCV's -- a print of it would not be read by the reference's detector (allow_fillers=True to print it anyway)")


def gen_svg(marker_id: int, dicno: int = 7, paper_size=PAPER["letter"], allow_fillers: bool = False) -> str:
    d = get_predefined_dictionary(dicno, allow_fillers=allow_fillers)
    _check_printable(d, marker_id, allow_fillers)
    black, white, lines, texts = page_layout(d, marker_id, paper_size)
    pw, ph = paper_size
    out = ['<svg width="%gmm" height="%gmm" viewBox="0 0 %g %g" version="1.1" xmlns="http://www.w3.org/2000/svg">' % (pw, ph, pw, ph)]
    for x, y, w, h in black:
        out.append('  <rect x="%.4f" y="%.4f" width="%.4f" height="%.4f" style="stroke:none; fill:black"/>' % (x, y, w, h))
    for x, y, w, h in white:
        out.append('  <rect class="cell" x="%.4f" y="%.4f" width="%.4f" height="%.4f" style="stroke:none; fill:white"/>' % (x, y, w, h))
    for x1, y1, x2, y2 in lines:
        out.append('  <line x1="%.4f" y1="%.4f" x2="%.4f" y2="%.4f" style="stroke:black; stroke-width:0.2"/>' % (x1, y1, x2, y2))
    for x, y, size, s in texts:
        out.append('  <text x="%.4f" y="%.4f" text-anchor="middle" style="font-family:arial; font-size:%gpt;">%s</text>' % (x, y, size * 25.4 / 72 * 0.75, s))
    out.append("</svg>")
    return "\n".join(out) + "\n"


def write_pdf(path: str, marker_ids, dicno: int = 7, paper_size=PAPER["letter"], allow_fillers: bool = False) -> None:
    """One marker per page, vector graphics, built-in Helvetica: a complete PDF 1.4 file written by hand."""
    d = get_predefined_dictionary(dicno, allow_fillers=allow_fillers)
    marker_ids = list(marker_ids)
    for mid in marker_ids:
        _check_printable(d, mid, allow_fillers)
    k = 72 / 25.4  # mm -> pt
    pw, ph = paper_size
    streams = []
    for mid in marker_ids:
        if not 0 <= mid < d.n_markers:
            raise ValueError(f"marker id {mid} not in {d.name}")
        black, white, lines, texts = page_layout(d, mid, paper_size)
        c = []

        def rect(x, y, w, h):
            c.append("%.3f %.3f %.3f %.3f re f" % (x * k, (ph - y - h) * k, w * k, h * k))

        c.append("0 g")
        for r in black:
            rect(*r)
        c.append("1 g")
        for r in white:
            rect(*r)
        c.append("0 G 0.5 w")
        for x1, y1, x2, y2 in lines:
            c.append("%.3f %.3f m %.3f %.3f l S" % (x1 * k, (ph - y1) * k, x2 * k, (ph - y2) * k))
        c.append("0 g")
        for x, y, size, s in texts:
            c.append(pdf_text(x, y, size, s, ph))
        streams.append("\n".join(c).encode("ascii"))
    with open(path, "wb") as fh:
        fh.write(pdf_file(streams, paper_size))


def pdf_file(page_streams, paper_size) -> bytes:
    """A complete PDF 1.4 file, one page of `paper_size` (mm) per content stream; the streams draw in points and may use the
    built-in Helvetica as /F1."""
    k = 72 / 25.4  # mm -> pt
    pw, ph = paper_size
    objs = []  # (object number -> bytes), numbered from 1

    def add(body: bytes) -> int:
        objs.append(body)
        return len(objs)

    font = add(b"<< /Type /Font /Subtype /Type1 /BaseFont /Helvetica >>")
    pages_id = 2 + 0  # reserved below
    add(b"")  # placeholder for /Pages (object 2)
    page_ids = []
    for stream in page_streams:
        content = add(b"<< /Length %d >>\nstream\n" % len(stream) + stream + b"\nendstream")
        page_ids.append(add(b"<< /Type /Page /Parent 2 0 R /MediaBox [0 0 %.3f %.3f] /Contents %d 0 R /Resources << /Font << /F1 %d 0 R >> >> >>"
                            % (pw * k, ph * k, content, font)))
    objs[pages_id - 1] = b"<< /Type /Pages /Kids [" + b" ".join(b"%d 0 R" % p for p in page_ids) + b"] /Count %d >>" % len(page_ids)
    catalog = add(b"<< /Type /Catalog /Pages 2 0 R >>")
    out = bytearray(b"%PDF-1.4\n%\xe2\xe3\xcf\xd3\n")
    offsets = []
    for i, body in enumerate(objs, 1):
        offsets.append(len(out))
        out += b"%d 0 obj\n" % i + body + b"\nendobj\n"
    xref = len(out)
    out += b"xref\n0 %d\n" % (len(objs) + 1) + b"0000000000 65535 f \n"
    for off in offsets:
        out += b"%010d 00000 n \n" % off
    out += b"trailer\n<< /Size %d /Root %d 0 R >>\nstartxref\n%d\n%%%%EOF\n" % (len(objs) + 1, catalog, xref)
    return bytes(out)


def pdf_text(x: float, y: float, size: float, s: str, page_height: float) -> str:
    """The content-stream operators of a label in Helvetica (/F1) of `size` pt, centred on x, baseline at y (mm, origin top left)."""
    k = 72 / 25.4  # mm -> pt
    width = 0.5 * size * len(s)  # Helvetica averages half an em per character: centred well enough for a label
    return "BT /F1 %g Tf %.3f %.3f Td (%s) Tj ET" % (size, x * k - width / 2, (page_height - y) * k, s.replace("(", "\\(").replace(")", "\\)"))


def charuco_sheet_layout(board, d: Dictionary, paper_size, allow_fillers: bool = False):
    """A ChArUco board (fiducials_amd.charuco.CharucoBoard, lengths in metres) as one page, printed at its true size and centred:
    (black rects, white rects, texts) in millimetres, origin top left.  The rectangles are board.layout()'s -- the board's own object
    points -- so the sheet and the pose tables agree by construction."""
    for i in board.ids:
        _check_printable(d, int(i), allow_fillers)
    pw, ph = paper_size
    bw, bh = board.squares_x * board.square_len * 1000.0, board.squares_y * board.square_len * 1000.0
    if bw > pw - 10 or bh > ph - 20:
        raise ValueError(f"a board of {bw:.1f} x {bh:.1f} mm does not fit a page of {pw} x {ph} mm with its margins")
    x0, y0 = (pw - bw) / 2, (ph - bh) / 2
    black, white = board.layout(d)

    def page(r):  # board metres, y up -> page mm, y down
        x, y, w, h = r
        return (x0 + x * 1000.0, y0 + bh - (y + h) * 1000.0, w * 1000.0, h * 1000.0)

    texts = [(pw / 2, y0 + bh + 8, 8, "ChArUco %d x %d, square %.2f mm, marker %.2f mm, ids %d - %d D%d: check the square size after printing."
              % (board.squares_x, board.squares_y, board.square_len * 1000.0, board.marker_len * 1000.0, board.ids[0], board.ids[-1], _dicno_of(d)))]
    return [page(r) for r in black], [page(r) for r in white], texts


def diamond_sheet_layout(diamond, d: Dictionary, paper_size, allow_fillers: bool = False):
    """A ChArUco diamond (fiducials_amd.charuco.CharucoDiamond) as one page -- the reference's drawCharucoDiamond: the sheet of its 3 x 3
    board, drawn from the diamond's own object points, under a label of its own."""
    black, white, texts = charuco_sheet_layout(diamond, d, paper_size, allow_fillers)
    x, y, size, _ = texts[0]
    label = "ChArUco diamond %s, square %.2f mm, marker %.2f mm D%d: check the square size after printing." % (
        ",".join(str(int(i)) for i in diamond.ids), diamond.square_len * 1000.0, diamond.marker_len * 1000.0, _dicno_of(d))
    return black, white, [(x, y, size, label)]


def _sheet_layout(board, d, paper_size, allow_fillers):
    from .charuco import CharucoDiamond

    return (diamond_sheet_layout if isinstance(board, CharucoDiamond) else charuco_sheet_layout)(board, d, paper_size, allow_fillers)


def gen_charuco_svg(board, dicno: int = 7, paper_size=PAPER["letter"], allow_fillers: bool = False) -> str:
    d = get_predefined_dictionary(dicno, allow_fillers=allow_fillers)
    black, white, texts = _sheet_layout(board, d, paper_size, allow_fillers)
    pw, ph = paper_size
    out = ['<svg width="%gmm" height="%gmm" viewBox="0 0 %g %g" version="1.1" xmlns="http://www.w3.org/2000/svg">' % (pw, ph, pw, ph)]
    for x, y, w, h in black:
        out.append('  <rect x="%.4f" y="%.4f" width="%.4f" height="%.4f" style="stroke:none; fill:black"/>' % (x, y, w, h))
    for x, y, w, h in white:
        out.append('  <rect class="cell" x="%.4f" y="%.4f" width="%.4f" height="%.4f" style="stroke:none; fill:white"/>' % (x, y, w, h))
    for x, y, size, s in texts:
        out.append('  <text x="%.4f" y="%.4f" text-anchor="middle" style="font-family:arial; font-size:%gpt;">%s</text>' % (x, y, size * 25.4 / 72 * 0.75, s))
    out.append("</svg>")
    return "\n".join(out) + "\n"


def write_charuco_pdf(path: str, board, dicno: int = 7, paper_size=PAPER["letter"], allow_fillers: bool = False) -> None:
    """The sheet as a one-page vector PDF."""
    d = get_predefined_dictionary(dicno, allow_fillers=allow_fillers)
    black, white, texts = _sheet_layout(board, d, paper_size, allow_fillers)
    k = 72 / 25.4
    ph = paper_size[1]
    c = ["0 g"] + ["%.3f %.3f %.3f %.3f re f" % (x * k, (ph - y - h) * k, w * k, h * k) for x, y, w, h in black]
    c += ["1 g"] + ["%.3f %.3f %.3f %.3f re f" % (x * k, (ph - y - h) * k, w * k, h * k) for x, y, w, h in white]
    c += ["0 g"] + [pdf_text(x, y, size, s, ph) for x, y, size, s in texts]
    with open(path, "wb") as fh:
        fh.write(pdf_file(["\n".join(c).encode("ascii")], paper_size))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Generate Aruco Markers.")
    ap.add_argument("startId", type=int, help="start of marker range to generate")
    ap.add_argument("endId", type=int, help="end of marker range to generate")
    ap.add_argument("out", type=str, help="PDF file to store the markers in (or a directory with --svg)")
    ap.add_argument("dictionary", type=int, default=7, nargs="?", help="dictionary to generate from")
    ap.add_argument("--paper-size", dest="paper_size", default="letter", choices=sorted(PAPER), help="paper size to use (letter or a4)")
    ap.add_argument("--svg", action="store_true", help="one self-contained SVG per marker into the directory `out`")
    ap.add_argument("--allow-fillers", action="store_true",
                    help="also print ids whose codeword in the shipped table is a locally generated filler (NOT OpenCV's: such a print "
                         "is only read back by this repository's own tables)")
    ap.add_argument("--charuco", metavar="SXxSY:SQUARE_MM:MARKER_MM",
                    help="one ChArUco board instead of single markers, e.g. 5x4:40:24; its markers are startId, startId + 1, ... (endId is not read)")
    ap.add_argument("--diamond", metavar="ID0,ID1,ID2,ID3[:SQUARE_MM:MARKER_MM]",
                    help="one ChArUco diamond instead of single markers, e.g. 0,1,1,2 (squares of 40 mm, markers of 24 mm) or "
                         "0,1,1,2:50:30; startId and endId are not read")
    a = ap.parse_args(argv)
    if a.charuco or a.diamond:
        from .charuco import CharucoBoard, CharucoDiamond

        if a.diamond:
            parts = a.diamond.split(":")
            if len(parts) not in (1, 3):
                ap.error("--diamond takes ID0,ID1,ID2,ID3 or ID0,ID1,ID2,ID3:SQUARE_MM:MARKER_MM")
            square, marker = parts[1:] if len(parts) == 3 else ("40", "24")
            board = CharucoDiamond([int(i) for i in parts[0].split(",")], float(square) / 1000.0, float(marker) / 1000.0)
            name = "diamond%s.svg" % "_".join(str(int(i)) for i in board.ids)
        else:
            size, square, marker = a.charuco.split(":")
            sx, sy = size.lower().split("x")
            board = CharucoBoard(int(sx), int(sy), float(square) / 1000.0, float(marker) / 1000.0, a.startId)
            name = "charuco%d.svg" % a.startId
        if a.svg:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, name), "w") as fh:
                fh.write(gen_charuco_svg(board, a.dictionary, PAPER[a.paper_size], a.allow_fillers))
        else:
            write_charuco_pdf(a.out, board, a.dictionary, PAPER[a.paper_size], a.allow_fillers)
        print("After printing, please make sure that a square is EXACTLY %.1f mm wide." % (board.square_len * 1000.0))
        return 0
    ids = list(range(a.startId, a.endId + 1))
    if a.svg:
        os.makedirs(a.out, exist_ok=True)
        for i in ids:
            with open(os.path.join(a.out, "marker%d.svg" % i), "w") as fh:
                fh.write(gen_svg(i, a.dictionary, PAPER[a.paper_size], a.allow_fillers))
    else:
        write_pdf(a.out, ids, a.dictionary, PAPER[a.paper_size], a.allow_fillers)
    print("After printing, please make sure that the long lines around the marker are EXACTLY 14.0cm long. "
          "This is required for accurate position estimation.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
