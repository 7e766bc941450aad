"""ChArUco boards (include/fid_abi.h, "ChArUco boards"): the board's geometry as the device library states it, in NumPy -- object points,
nearest-marker tables, the board as a map for the marker-corner entry points, and a raster for tests and synthetic frames.  Host code;
the interpolation, refinement and pose run on the device through ArucoDetector.set_charuco_board / charuco_last / charuco_pose*."""
from __future__ import annotations

import numpy as np

from . import _lib
from .dictionary import Dictionary, draw_marker


def _f32(v):
    """a double rounded through float (Point3f)"""
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


class CharucoBoard:
    """squares_x x squares_y squares of square_len, a marker of marker_len in every white square (x + y odd), ids first_id, first_id +
    1, ... over the white squares with y outermost.  Board frame: x right, y up, z out of the face; square (x, y) covers
    [x s, (x + 1) s] x [y s, (y + 1) s]."""

    def __init__(self, squares_x: int, squares_y: int, square_len: float, marker_len: float, first_id: int = 0):
        self.squares_x, self.squares_y = int(squares_x), int(squares_y)
        self.square_len, self.marker_len, self.first_id = float(square_len), float(marker_len), int(first_id)
        if self.squares_x < 2 or self.squares_y < 2:
            raise ValueError("a ChArUco board has at least 2 squares a side")
        if not 0 < self.marker_len < self.square_len:
            raise ValueError("marker_len must lie inside (0, square_len)")
        sx, sy, s, m = self.squares_x, self.squares_y, self.square_len, self.marker_len
        d = (s - m) / 2
        # the white squares in marker order, and the marker index of every square (-1: black)
        self.marker_squares = np.array([(x, y) for y in range(sy) for x in range(sx) if (x + y) % 2 == 1], np.int64).reshape(-1, 2)
        self.marker_at = np.full((sy, sx), -1, np.int64)
        for k, (x, y) in enumerate(self.marker_squares):
            self.marker_at[y, x] = k
        self.n_markers = len(self.marker_squares)
        self.ids = (self.first_id + np.arange(self.n_markers)).astype(np.int32)
        obj = np.zeros((self.n_markers, 4, 3))
        for k, (x, y) in enumerate(self.marker_squares):
            c0x, c0y = x * s + d, y * s + d + m
            obj[k, :, 0] = (c0x, c0x + m, c0x + m, c0x)
            obj[k, :, 1] = (c0y, c0y, c0y - m, c0y - m)
        self.marker_object_points = _f32(obj)  # (n_markers, 4, 3)
        self.n_corners = (sx - 1) * (sy - 1)
        cobj = np.zeros((self.n_corners, 3))
        self.corner_grid = np.zeros((self.n_corners, 2), np.int64)  # (cx, cy) of every chessboard corner
        self.nearest_markers = np.zeros((self.n_corners, 2), np.int64)
        self.nearest_corners = np.zeros((self.n_corners, 2), np.int64)
        for cy in range(sy - 1):
            for cx in range(sx - 1):
                i = cy * (sx - 1) + cx
                self.corner_grid[i] = (cx, cy)
                cobj[i] = ((cx + 1) * s, (cy + 1) * s, 0.0)
        self.corner_object_points = _f32(cobj)  # (n_corners, 3)
        for i, (cx, cy) in enumerate(self.corner_grid):
            sq = ((cx + 1, cy), (cx, cy + 1)) if (cx + cy) % 2 == 0 else ((cx, cy), (cx + 1, cy + 1))
            mk = sorted(int(self.marker_at[y, x]) for x, y in sq)
            self.nearest_markers[i] = mk
            for w, k in enumerate(mk):
                dd = ((self.marker_object_points[k, :, :2] - self.corner_object_points[i, :2]) ** 2).sum(axis=1)
                self.nearest_corners[i, w] = int(np.argmin(dd))

    def c_struct(self) -> "_lib.FidCharucoBoard":
        return _lib.FidCharucoBoard(self.squares_x, self.squares_y, self.square_len, self.marker_len, self.first_id, 0)

    def as_map_entries(self) -> np.ndarray:
        """The board's markers as fid_map_entry records (detector.MAP_ENTRY_DTYPE) for set_map / map_pose*: len = marker_len, no
        rotation, t = the marker's centre.  fid_set_map rebuilds the corners as t -+ (double)(float)(len / 2): they are the board's own
        object points exactly when the lengths are exact in float (dyadic), and within a float rounding of them otherwise."""
        from .detector import map_entries

        centre = 0.5 * (self.marker_object_points[:, 0] + self.marker_object_points[:, 2])
        return map_entries(self.ids, self.marker_len, np.broadcast_to(np.eye(3), (self.n_markers, 3, 3)), centre)

    def layout(self, d: Dictionary, border_bits: int = 1):
        """The board as rectangles in board coordinates, from the same object points the pose uses: (black, white), each a list of
        (x, y, w, h) with (x, y) the corner of least x and y.  Black: the black squares and every marker's square; white: the white
        cells of every marker, on top."""
        s = self.square_len
        black = [(x * s, y * s, s, s) for y in range(self.squares_y) for x in range(self.squares_x) if (x + y) % 2 == 0]
        white = []
        ncell = d.marker_size + 2 * border_bits
        for k in range(self.n_markers):
            c0, c2 = self.marker_object_points[k, 0], self.marker_object_points[k, 2]  # top left, bottom right
            w, h = c2[0] - c0[0], c0[1] - c2[1]
            black.append((c0[0], c2[1], w, h))
            cells = draw_marker(d, int(self.ids[k]), ncell, border_bits)
            for r in range(ncell):
                for c in range(ncell):
                    if cells[r, c] > 0:
                        white.append((c0[0] + c * w / ncell, c0[1] - (r + 1) * h / ncell, w / ncell, h / ncell))
        return black, white

    def draw(self, d: Dictionary, px_per_square: int, border_bits: int = 1) -> np.ndarray:
        """The board as a raster (row 0 is the board's top edge, y = squares_y s): uint8, 0 black / 255 white, px_per_square pixels a
        square, every marker drawn (drawMarker semantics, nearest neighbour) into the pixels its object points cover."""
        pps = int(px_per_square)
        Hpx, Wpx = self.squares_y * pps, self.squares_x * pps
        img = np.full((Hpx, Wpx), 255, np.uint8)
        k = pps / self.square_len
        for x in range(self.squares_x):
            for y in range(self.squares_y):
                if (x + y) % 2 == 0:
                    img[Hpx - (y + 1) * pps:Hpx - y * pps, x * pps:(x + 1) * pps] = 0
        for m in range(self.n_markers):
            c0, c2 = self.marker_object_points[m, 0], self.marker_object_points[m, 2]
            x0, x1 = int(round(c0[0] * k)), int(round(c2[0] * k))
            y0, y1 = Hpx - int(round(c0[1] * k)), Hpx - int(round(c2[1] * k))
            img[y0:y1, x0:x1] = draw_marker(d, int(self.ids[m]), x1 - x0, border_bits)[:y1 - y0]
        return img


class CharucoDiamond(CharucoBoard):
    """A ChArUco diamond (include/fid_abi.h, "ChArUco diamonds"): the 3 x 3 board whose four markers, in the squares (1,0), (0,1), (2,1),
    (1,2), carry the ids given -- any four, repeats allowed -- around the black middle square.  Object points, layout() and draw() are
    the board's, so the printed sheet (marker_gen --diamond), the synthetic frame (synth.make_diamond_frame) and the pose agree by
    construction.  ArucoDetector.diamonds_last reports the chessboard corners in the order RECORD_CORNERS."""

    RECORD_CORNERS = (2, 3, 1, 0)  # fid_diamond.corners: the order of a marker's corners (top left, top right, bottom right, bottom left)

    def __init__(self, ids, square_len: float, marker_len: float):
        super().__init__(3, 3, square_len, marker_len, 0)
        ids = np.asarray(ids, np.int64).reshape(-1)
        if len(ids) != 4 or np.any(ids < 0):
            raise ValueError("a diamond has four marker ids, none negative")
        self.ids = ids.astype(np.int32)

    @property
    def square_marker_rate(self) -> float:
        return self.square_len / self.marker_len

    @property
    def record_object_points(self) -> np.ndarray:
        """(4, 3): the chessboard corners in the order of fid_diamond.corners"""
        return self.corner_object_points[list(self.RECORD_CORNERS)]

    @property
    def centre(self) -> np.ndarray:
        """the middle of the middle square: the origin of the fiducial that diamond_pose poses"""
        return np.array([1.5 * self.square_len, 1.5 * self.square_len, 0.0])

    def c_struct(self):
        raise TypeError("a diamond is not a context's board: diamonds_last / diamonds_detect take its square_marker_rate")
