"""The diamond entry points (include/fid_abi.h: "ChArUco diamonds") restated in NumPy from the header's text, steps 1 - 5: proposals,
resolution, positions, windows and selection, refinement (oracle.corner_subpix one corner at a time), the record.  The homography is
charuco_restatement.homography4 -- exact, where the device uses the closed form -- and the window and the refinement are that module's.
detect() also returns the MARGIN of every decision the matching takes, so that a set of cases can prove on the CPU that no float
rounding on the device can flip one.  No test of its own; tests/test_diamond_restatement.py (CPU) and tests/test_gpu_diamond.py use it."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import charuco_restatement as cr

MAX_PER_FRAME, MAX_MARKERS = 64, 256
RECORD_CORNERS = (2, 3, 1, 0)  # the chessboard corners in the order of fid_diamond.corners
DEFAULT_RATE, DEFAULT_MAX_REP_RATE = 0.04 / 0.024, 1.0


def layout(rate: float) -> cr.Board:
    """L(rate): the 3 x 3 board with marker_len = 1, square_len = rate"""
    b = cr.Board(3, 3, float(rate), 1.0)
    assert b.n_markers == 4 and b.n_corners == 4
    return b


def side(c) -> float:
    """the mean of a marker's four side lengths: the difference in float, the norm in double"""
    c = np.asarray(c, np.float32).reshape(4, 2)
    tot = 0.0
    for i in range(4):
        d = c[i] - c[(i + 1) % 4]
        tot += float(np.sqrt(np.float64(d[0]) * np.float64(d[0]) + np.float64(d[1]) * np.float64(d[1])))
    return tot / 4.0


def _through(h, pts) -> np.ndarray:
    """(n, 2) plane points through the homography h, each coordinate rounded to float"""
    q = np.concatenate([np.asarray(pts, np.float64)[:, :2], np.ones((len(pts), 1))], axis=1) @ h.T
    return (q[:, :2] / q[:, 2:3]).astype(np.float32)


def _d2(q, corners) -> np.ndarray:
    """d2(k, j) for every j: the maximum over the four corners, in the same order, of dx^2 + dy^2 (float difference, double square)"""
    diff = (q[None] - corners).astype(np.float64)  # q, corners float32: the subtraction is made in float
    return (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]).max(axis=1)


@dataclass
class Margins:
    tol: list = field(default_factory=list)  # |d - tol_a| / tol_a of every best candidate, accepted or rejected
    gap: list = field(default_factory=list)  # (second-best d - best d) / tol_a of every accepted best candidate (a rejected one decides nothing)

    def worst(self) -> float:
        return min(self.tol + self.gap) if self.tol or self.gap else np.inf


def proposals(L: cr.Board, max_rep_rate: float, corners, margins: Margins | None = None) -> list:
    """Step 1 -> per marker a: (m_1, m_2, m_3), or None where the proposal is not valid"""
    corners = np.asarray(corners, np.float32).reshape(-1, 4, 2)
    n = len(corners)
    out = []
    for a in range(n):
        h = cr.homography4(L.marker_obj[0, :, :2], corners[a].astype(np.float64))
        if h is None or not np.all(np.isfinite(h)) or n < 2:
            out.append(None)
            continue
        tol = float(max_rep_rate) * side(corners[a])
        ms, valid = [], True
        for k in (1, 2, 3):
            d2 = _d2(_through(h, L.marker_obj[k]), corners)
            d2[a] = np.inf
            m = int(np.argmin(d2))  # (the first of equal values: the lower j)
            d = float(np.sqrt(d2[m]))
            if margins is not None:
                margins.tol.append(abs(d - tol) / tol)
                if d2[m] < tol * tol and n > 2:
                    margins.gap.append(float(np.sqrt(np.partition(d2, 1)[1]) - d) / tol)
            valid = valid and bool(d2[m] < tol * tol)
            ms.append(m)
        out.append(tuple(ms) if valid and len(set(ms)) == 3 else None)
    return out


def resolve(props) -> list:
    """Step 2 -> the founded diamonds (a, m_1, m_2, m_3) in the order of their anchors"""
    taken, found = set(), []
    for a, p in enumerate(props):
        if p is None or a in taken or any(m in taken for m in p) or len(found) >= MAX_PER_FRAME:
            continue
        taken.update((a,) + p)
        found.append((a,) + p)
    return found


def positions(L: cr.Board, corners, members):
    """Step 3 for one diamond -> (positions float32 (4, 2) by chessboard corner, windows (4,)), or None without a homography"""
    corners = np.asarray(corners, np.float32).reshape(-1, 4, 2)
    Hk = []
    for k, m in enumerate(members):
        h = cr.homography4(L.marker_obj[k, :, :2], corners[m].astype(np.float64))
        if h is None or not np.all(np.isfinite(h)):
            return None
        Hk.append(h)
    pos, wins = np.zeros((4, 2), np.float32), np.zeros(4, np.int64)
    for i in range(4):
        ps = [_through(Hk[int(k)], L.corner_obj[i:i + 1])[0] for k in L.near_marker[i]]
        pos[i] = (ps[0] + ps[1]) / np.float32(2)
        wins[i] = device_window(L, corners, members, i, pos[i])
    return pos, wins


def device_window(L: cr.Board, corners, members, i: int, p) -> int:
    """rule 3 for chessboard corner i of the diamond `members` at the position p"""
    corners = np.asarray(corners, np.float32).reshape(-1, 4, 2)
    return cr.window(p, [corners[members[int(k)], int(c)] for k, c in zip(L.near_marker[i], L.near_corner[i])])


def detect(rate, max_rep_rate, ids, corners, W, H, gray=None, refine=True):
    """Steps 1 - 5 -> (records, margins).  A record is a dict with the fields of fid_diamond."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    corners = np.asarray(corners, np.float32).reshape(-1, 4, 2)
    assert len(ids) == len(corners) <= MAX_MARKERS
    L, mg = layout(rate), Margins()
    recs = []
    for members in resolve(proposals(L, max_rep_rate, corners, mg)):
        pw = positions(L, corners, members)
        if pw is None:
            continue
        pos, wins = pw
        if not all(2 <= p[0] < W - 2 and 2 <= p[1] < H - 2 for p in pos):
            continue  # (not reported; its markers stay assigned)
        order = list(RECORD_CORNERS)
        c0, w = pos[order], wins[order]
        c = cr.refine(gray, c0, w) if refine and gray is not None else c0.copy()
        recs.append({"ids": ids[list(members)].astype(np.int32), "index": np.array(members, np.int32), "corners": c, "corners0": c0, "win": w})
    return recs, mg
