"""Frames on which marker identification has something to decide, and the plain statement of what it must decide.

Every other frame of the suite carries clean codewords on dense histograms: an accepted candidate sits at Hamming distance 0, a
rejected one is clutter.  The frames here put candidates ON the limits of `_identifyOneCandidate` / `Dictionary::identify`
(aruco.cpp, dictionary.cpp):

  family 1  data-bit errors 0 ... maxCorr + 1 in every frame, five codeword sizes, three errorCorrectionRates;
  family 2  a word within capacity of several table entries: the FIRST such entry wins, across the 64-marker rounds and the
            256-marker table fetches of the device's search, with a partial last round and a rotation tie;
  family 3  white cells in the inner ring of a two-cell border: 0, limit - 1, limit, limit + 1 of them in one frame;
  family 4  flat scenes without blur or noise: two grey levels in a marker, one behind it -- sparse Otsu histograms whose
            occupied bins sit on and beside the 64-bin word edges;
  batches   three frames under one parameter set, for the batch entry point.

The reference here is numpy and nothing else: no device code and no oracle call.  tests/test_identify_cases.py holds the
oracle to it on every frame (and shows that no frame is vacuous); tests/test_gpu_identify_damaged.py holds the device to both."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from fiducials_amd.dictionary import Dictionary, bits_from_bytes, byte_list_from_bits, get_predefined_dictionary
from fiducials_amd.synth import make_frame

CORNER_MATCH_PX = 3.0  # a candidate / detection belongs to a drawn marker when its four corners are this close to the drawn ones


# ---------------------------------------------------------------------------------------------- the plain reference
def max_corr(d: Dictionary, rate: float) -> int:
    """Dictionary::identify: maxCorrectionRecalculed."""
    return int(float(d.max_correction_bits) * rate)


def max_border(marker_size: int, rate: float) -> int:
    """_identifyOneCandidate: maximumErrorsInBorder."""
    return int(marker_size * marker_size * rate)


def identify_plain(d: Dictionary, bits: np.ndarray, max_corr_bits: int):
    """Dictionary::identify: (id, rotation) of the FIRST marker whose best rotation is within max_corr_bits of `bits`, the
    first of equally good rotations; (-1, -1) if there is none."""
    n = d.marker_size
    bits = np.asarray(bits, dtype=np.uint8).reshape(n, n)
    h = (_table_bits(d) != bits).sum(axis=(2, 3))    # (nMarkers, 4) Hamming distances
    within = np.flatnonzero(h.min(axis=1) <= max_corr_bits)
    if len(within) == 0:
        return -1, -1
    m = int(within[0])                                 # the first, not the nearest
    return m, int(np.argmin(h[m]))                     # (argmin: the first of equal rotations)


_TABLES: dict = {}


def _table_bits(d: Dictionary) -> np.ndarray:
    """bits_from_bytes of every entry and rotation, (nMarkers, 4, n, n), unpacked once per byte table."""
    key = (d.marker_size, d.bytes_list.tobytes())
    if key not in _TABLES:
        _TABLES[key] = np.stack([np.stack([bits_from_bytes(d.bytes_list[m, r], d.marker_size) for r in range(4)]) for m in range(d.n_markers)])
    return _TABLES[key]


def expected_id(d: Dictionary, bits: np.ndarray, max_corr_bits: int) -> int:
    return identify_plain(d, bits, max_corr_bits)[0]


def border_errors(grid: np.ndarray, marker_size: int, border_bits: int) -> int:
    """_getBorderErrors: the white cells among the border cells of a (n + 2b)^2 grid."""
    g = np.asarray(grid) != 0
    b = border_bits
    return int(g.sum() - g[b:b + marker_size, b:b + marker_size].sum())


def full_grid(bits: np.ndarray, border_bits: int) -> np.ndarray:
    """drawMarker's cell grid, 0 / 255: the data bits inside border_bits cells of black."""
    n = bits.shape[0]
    g = np.zeros((n + 2 * border_bits,) * 2, np.uint8)
    g[border_bits:border_bits + n, border_bits:border_bits + n] = (np.asarray(bits) != 0) * 255
    return g


def flip_bits(bits: np.ndarray, k: int, rng) -> np.ndarray:
    out = np.array(bits, dtype=np.uint8).copy()
    pos = rng.choice(out.size, size=k, replace=False)
    out.reshape(-1)[pos] ^= 1
    return out


def print_dictionary(d: Dictionary, words) -> Dictionary:
    """The 'print' dictionary: entry j is the (possibly damaged) word that marker j of a frame is drawn with."""
    bl = np.ascontiguousarray(np.stack([byte_list_from_bits(np.asarray(w, dtype=np.uint8)) for w in words]))
    return Dictionary("print", d.marker_size, d.max_correction_bits, bl, np.zeros(len(words), bool))


def match_drawn(drawn: np.ndarray, quad: np.ndarray, tol: float = CORNER_MATCH_PX):
    """Index of the drawn marker whose corners are the quad's (any starting corner, either direction), or None."""
    q = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    for j, g in enumerate(drawn):
        for cand in (q, q[::-1]):
            for s in range(4):
                if np.abs(np.roll(cand, s, axis=0) - g).max() <= tol:
                    return j
    return None


# ---------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    family: int
    d: Dictionary            # what the detector holds (the TRUE dictionary)
    params: dict             # DetectorParameters away from the node defaults, the same on every side
    image: np.ndarray
    corners: np.ndarray      # (M, 4, 2) drawn corners
    bits: np.ndarray         # (M, n, n) drawn data bits
    border_white: np.ndarray  # (M,) white cells in the drawn border
    must_read: bool = True   # every drawn marker within both limits is read (False: only "nothing wrong is read" is claimed)
    uniform: bool = False    # the patch's standard deviation is below minOtsuStdDev: nothing is read
    expected: np.ndarray = field(default=None)  # (M,) the id each drawn marker must get, -1: rejected
    wanted: list = None      # family 2: the ids the case was built to give, marker by marker (the plain rule is held to them)

    def __post_init__(self):
        rate = self.params.get("errorCorrectionRate", 0.6)
        brate = self.params.get("maxErroneousBitsInBorderRate", 0.04)
        mc, mb = max_corr(self.d, rate), max_border(self.d.marker_size, brate)
        exp = []
        for b, w in zip(self.bits, self.border_white):
            exp.append(-1 if (self.uniform or w > mb) else expected_id(self.d, b, mc))
        self.expected = np.array(exp, dtype=np.int32)

    @property
    def size(self):
        return self.image.shape[1], self.image.shape[0]

    def counts(self):
        """(drawn, read, rejected) by the plain rule."""
        return len(self.expected), int((self.expected >= 0).sum()), int((self.expected < 0).sum())


def check_against_rule(case: Case, ids, corners) -> dict:
    """A detector's answer on the frame against the plain rule, marker by marker: every returned marker is a drawn one, carries
    the id the rule gives it, and none beyond a limit appears; where the case says so, every marker within the limits is there."""
    seen = {}
    for i, c in zip(np.asarray(ids).tolist(), np.asarray(corners)):
        j = match_drawn(case.corners, c)
        assert j is not None, f"{case.name}: id {i} at {c.tolist()} is no drawn marker"
        assert j not in seen, f"{case.name}: drawn marker {j} returned twice"
        assert case.expected[j] >= 0, f"{case.name}: drawn marker {j} is beyond a limit and was returned as id {i}"
        assert i == case.expected[j], f"{case.name}: drawn marker {j} returned as id {i}, the rule says {case.expected[j]}"
        seen[j] = i
    if case.must_read:
        want = sorted(int(e) for e in case.expected if e >= 0)
        assert sorted(np.asarray(ids).tolist()) == want, f"{case.name}: ids {sorted(np.asarray(ids).tolist())}, the rule says {want}"
    return seen


# ---- family 1
# Sensor noise 0.5 instead of make_frame's 2.0: a black border wider than the threshold window is thresholded to an outline, whose
# inner edge (a second quad 3 ... 12 px inside the drawn one, on flat black where noise alone decides the pixels) competes with
# the outer edge in _filterTooCloseCandidates by contour length; at sigma 2 the ragged inner one wins for a quarter of the markers
# and the candidate is no longer the drawn quad.  At 0.5 the outer contour wins everywhere and the drawn corners can be asserted.
NOISE = 0.5
F1_FRAME = dict(width=1280, height=720, n_markers=12, side_range=(90.0, 140.0), max_tilt_deg=25.0, noise_sigma=NOISE)
FAMILY1 = [("DICT_4X4_50", 0.6), ("DICT_4X4_50", 1.0), ("DICT_5X5_50", 0.0), ("DICT_5X5_50", 0.6), ("DICT_5X5_50", 1.0),
           ("DICT_5X5_250", 0.6), ("DICT_5X5_250", 1.0), ("DICT_6X6_50", 0.6), ("DICT_6X6_50", 1.0), ("DICT_7X7_50", 0.6),
           ("DICT_7X7_50", 1.0)]


F1_SEEDS = {("DICT_7X7_50", 1.0): 1000}   # (dictionary, rate) -> seed, where 900 + k does not satisfy the condition of test_identify_cases.py


def _damaged_frame(name, family, d, params, seed, border_bits=1, frame=F1_FRAME):
    """Marker j carries j mod (maxCorr + 2) flipped data bits: every distance 0 ... maxCorr + 1 occurs."""
    mc = max_corr(d, params.get("errorCorrectionRate", 0.6))
    rng = np.random.default_rng(seed)
    m = frame["n_markers"]
    ids = rng.choice(d.n_markers, size=m, replace=False)
    words = [flip_bits(d.bits(int(ids[j])), j % (mc + 2), rng) for j in range(m)]
    fr = make_frame(print_dictionary(d, words), seed, ids=np.arange(m), border_bits=border_bits, **frame)
    return Case(name, family, d, params, fr.image, fr.corners, np.stack(words), np.zeros(m, np.int32))


@functools.lru_cache(maxsize=None)
def family1_case(k: int) -> Case:
    name, rate = FAMILY1[k]
    d = get_predefined_dictionary(name, allow_fillers=True)
    return _damaged_frame(f"f1-{name}-{rate}", 1, d, dict(errorCorrectionRate=rate), F1_SEEDS.get((name, rate), 900 + k))


# ---- family 2
F2_FRAME = dict(width=1280, height=720, n_markers=8, side_range=(150.0, 200.0), max_tilt_deg=10.0, noise_sigma=NOISE)
F2_ENTRIES = 300   # no multiple of 64: the last round of the search is partial
F2_W_FROM = 500    # w: an entry of the 1000-entry table beyond the first 300
FAMILY2 = [(5, True), (5, False), (6, True), (6, False)]   # (marker size, entry 70 overwritten)
F2_SEEDS = {2: 1002, 3: 1002}   # k -> seed, where 920 + k does not satisfy the condition of test_identify_cases.py


@functools.lru_cache(maxsize=None)
def family2_dictionary(n: int, with_70: bool):
    """300 entries of the n x n table, maxCorrectionBits 2.  Entry 70 <- w with two flips (if with_70), 130 <- w with one flip,
    260 <- w (behind the first 256-marker fetch), 299 <- a word that is its own half turn.  Returns (dictionary, w, symmetric)."""
    big = get_predefined_dictionary({5: "DICT_5X5_1000", 6: "DICT_6X6_1000"}[n], allow_fillers=True)
    rng = np.random.default_rng(70 + n)
    w = big.bits(F2_W_FROM)
    bl = big.bytes_list[:F2_ENTRIES].copy()
    if with_70:
        bl[70] = byte_list_from_bits(flip_bits(w, 2, rng))
    bl[130] = byte_list_from_bits(flip_bits(w, 1, rng))
    bl[260] = byte_list_from_bits(w)
    sym = rng.integers(0, 2, (n, n)).astype(np.uint8)
    flat = sym.reshape(-1)
    for k in range(n * n // 2):
        flat[n * n - 1 - k] = flat[k]
    assert np.array_equal(sym, np.rot90(sym, 2))
    bl[299] = byte_list_from_bits(sym)
    d = Dictionary(f"custom_{n}x{n}_{F2_ENTRIES}" + ("" if with_70 else "_no70"), n, 2, np.ascontiguousarray(bl), np.zeros(F2_ENTRIES, bool))
    return d, w, sym


def family2_words(n: int, with_70: bool, seed: int):
    """(words printed, the id each must get): w itself, the symmetric word, entry 298 with one flip, and clean entries on the
    lane and round edges of the search."""
    d, w, sym = family2_dictionary(n, with_70)
    rng = np.random.default_rng(seed)
    words = [w, sym, flip_bits(d.bits(298), 1, rng)] + [d.bits(i) for i in (0, 63, 64, 255, 256)]
    return d, words, [70 if with_70 else 130, 299, 298, 0, 63, 64, 255, 256]


@functools.lru_cache(maxsize=None)
def family2_case(k: int, seed: int = 0) -> Case:
    n, with_70 = FAMILY2[k]
    seed = seed or F2_SEEDS.get(k, 920 + k)
    d, words, want = family2_words(n, with_70, seed)
    fr = make_frame(print_dictionary(d, words), seed, ids=np.arange(len(words)), **F2_FRAME)
    return Case(f"f2-{d.name}-{seed}", 2, d, dict(errorCorrectionRate=1.0), fr.image, fr.corners, np.stack(words),
                np.zeros(len(words), np.int32), wanted=want)


# ---- family 3
F3_FRAME = dict(width=1280, height=720, n_markers=8, side_range=(170.0, 220.0), max_tilt_deg=10.0, noise_sigma=NOISE)
F3_RATES = (0.04, 0.15, 0.35)
F3_DICTS = ("DICT_4X4_50", "DICT_5X5_250", "DICT_6X6_250", "DICT_7X7_50")
FAMILY3 = [(name, rate) for name in F3_DICTS for rate in F3_RATES]
F3_SEEDS = {}   # (dictionary, rate) -> seed, where 940 + k does not satisfy the condition of test_identify_cases.py
# minMarkerDistanceRate 0.02 instead of 0.05: the dark halo the background forms around make_frame's one-cell white quiet zone is a
# quad of its own, sqrt(2) cells from the marker's corners.  With a two-cell border that is sqrt(2) / (n + 4) of a side -- 0.13 for
# 7 x 7 -- while _filterTooCloseCandidates merges candidates closer than 0.05 x contour length = 0.14 ... 0.2 of a side and keeps the
# longer contour: the halo.  Every 10- and 11-cell marker would lose its candidate, whatever seed, size or tilt.  At 0.02 (0.06 ... 0.08
# of a side) the halo stays a candidate of its own (it is read and rejected) and the marker's outline keeps its drawn corners.
F3_PARAMS = dict(markerBorderBits=2, minMarkerDistanceRate=0.02)


def inner_ring(n: int):
    """The cells of the inner ring of a two-cell border around n x n data cells, as (row, column) in the (n + 4)^2 grid."""
    lo, hi = 1, n + 2
    return [(r, c) for r in range(lo, hi + 1) for c in range(lo, hi + 1) if r in (lo, hi) or c in (lo, hi)]


def _border_frame(name, family, d, params, seed, ids=None, words=None, frame=F3_FRAME):
    """Two-cell borders with white cells in the INNER ring only (the outline, and with it the candidate, stays whole): per frame
    0, limit - 1, limit and limit + 1 of them (never below 0), twice over."""
    n = d.marker_size
    mb = max_border(n, params.get("maxErroneousBitsInBorderRate", 0.04))
    rng = np.random.default_rng(seed)
    m = frame["n_markers"]
    if ids is None:
        ids = rng.choice(d.n_markers, size=m, replace=False)
        words = [d.bits(int(i)) for i in ids]
    ring = inner_ring(n)
    grids, white = {}, []
    for j in range(m):
        k = max(0, (0, mb - 1, mb, mb + 1)[j % 4])
        g = full_grid(words[j], 2)
        for q in rng.choice(len(ring), size=k, replace=False):
            g[ring[q]] = 255
        grids[j] = g
        white.append(border_errors(g, n, 2))
    fr = make_frame(print_dictionary(d, words), seed, ids=np.arange(m), border_bits=2, cells=grids, **frame)
    return Case(name, family, d, params, fr.image, fr.corners, np.stack(words), np.array(white, np.int32))


@functools.lru_cache(maxsize=None)
def family3_case(k: int) -> Case:
    name, rate = FAMILY3[k]
    d = get_predefined_dictionary(name, allow_fillers=True)
    return _border_frame(f"f3-{name}-{rate}", 3, d, dict(F3_PARAMS, maxErroneousBitsInBorderRate=rate), F3_SEEDS.get((name, rate), 940 + k))


# ---- family 4
F4_LEVELS = [(0, 255, 128), (0, 1, 255), (63, 64, 255), (127, 128, 255), (191, 192, 255), (100, 101, 140), (64, 200, 255),
             (0, 64, 255), (63, 255, 160), (25, 230, 255), (10, 247, 255), (3, 250, 120)]   # (black, white, background)
# three marker levels: the white cells alternate between two levels (black, white a, white b, background)
F4_LEVELS3 = [(0, 254, 255, 128), (63, 191, 192, 255), (1, 128, 129, 255), (64, 127, 128, 200)]
F4_DICT = "DICT_5X5_250"
F4_IDS = (3, 17, 64, 101, 200, 249)
F4_CELL = 16          # pixels a cell: 7 cells = 112 px a side
F4_ROTATION = 0.13    # rad per marker in the rotated scenes: marker j is turned by (j + 1) * 0.13


def flat_scene(d: Dictionary, ids, levels, rotation: float, width=640, height=480, cell=F4_CELL):
    """Markers on a flat background, no quiet zone of their own, no blur, no noise, nearest neighbour: the pixel whose centre
    falls into a cell takes the cell's level.  levels: (black, white, background) or (black, white a, white b, background).
    Returns (image, drawn corners TL TR BR BL, data bits)."""
    black, bg = levels[0], levels[-1]
    whites = levels[1:-1]
    n = d.marker_size
    nc = n + 2
    side = nc * cell
    img = np.full((height, width), bg, np.uint8)
    cols, rows = 3, 2
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    corners, bits = [], []
    for j, mid in enumerate(ids):
        cx = (j % cols + 0.5) * width / cols - 0.5
        cy = (j // cols + 0.5) * height / rows - 0.5
        a = rotation * (j + 1)
        ca, sa = np.cos(a), np.sin(a)
        # image -> marker coordinates in cells, origin at the marker's top-left corner
        u = (ca * (xx - cx) + sa * (yy - cy)) / cell + nc / 2
        v = (-sa * (xx - cx) + ca * (yy - cy)) / cell + nc / 2
        inside = (u >= 0) & (u < nc) & (v >= 0) & (v < nc)
        ui, vi = np.clip(np.floor(u).astype(np.int64), 0, nc - 1), np.clip(np.floor(v).astype(np.int64), 0, nc - 1)
        b = d.bits(int(mid))
        grid = np.full((nc, nc), black, np.uint8)
        for r in range(n):
            for c in range(n):
                if b[r, c]:
                    grid[r + 1, c + 1] = whites[(r + c) % len(whites)]
        img = np.where(inside, grid[vi, ui], img)
        h = side / 2
        local = np.array([[-h, -h], [h, -h], [h, h], [-h, h]])
        corners.append(local @ np.array([[ca, sa], [-sa, ca]]) + (cx, cy))
        bits.append(b)
    return img.astype(np.uint8), np.array(corners), np.stack(bits)


def _adjacent(levels):
    return max(levels[:-1]) - min(levels[:-1]) <= 1


FAMILY4 = [(lv, rot, sd) for lv in F4_LEVELS + F4_LEVELS3 for rot in (False, True) for sd in (0.0, 5.0)]


@functools.lru_cache(maxsize=None)
def _family4_scene(levels, rotated):
    return flat_scene(get_predefined_dictionary(F4_DICT), F4_IDS, levels, F4_ROTATION if rotated else 0.0)


@functools.lru_cache(maxsize=None)
def family4_case(k: int) -> Case:
    levels, rotated, sd = FAMILY4[k]
    d = get_predefined_dictionary(F4_DICT)
    img, corners, bits = _family4_scene(levels, rotated)
    # adjacent marker levels under the default minOtsuStdDev: an axis-aligned patch is uniform and nothing is read; a rotated
    # patch pulls background in, so some go down the Otsu path -- there only "nothing wrong is read" is claimed
    uniform = _adjacent(levels) and sd > 0 and not rotated
    must = not rotated and not uniform
    return Case(f"f4-{'-'.join(map(str, levels))}-{'rot' if rotated else 'flat'}-sd{sd:g}", 4, d, dict(minOtsuStdDev=sd), img, corners, bits,
                np.zeros(len(bits), np.int32), must_read=must, uniform=uniform)


# ---- batches: three frames under ONE parameter set, so that one detect_markers_batch call holds them
BATCH_GROUPS = ["borders-5x5", "first-hit-5x5"]


@functools.lru_cache(maxsize=None)
def batch_group(name: str):
    """(dictionary, parameters, [three cases])."""
    if name == "borders-5x5":
        # data-bit damage and border damage under the same two-cell-border parameters
        d = get_predefined_dictionary("DICT_5X5_250")
        p = dict(F3_PARAMS, maxErroneousBitsInBorderRate=0.15, errorCorrectionRate=1.0)
        cases = [_damaged_frame("b1-bits-a", 5, d, p, 960, border_bits=2, frame=F3_FRAME),
                 _border_frame("b1-border", 5, d, p, 961),
                 _damaged_frame("b1-bits-b", 5, d, p, 962, border_bits=2, frame=F3_FRAME)]
        return d, p, cases
    if name == "first-hit-5x5":
        d = family2_dictionary(5, True)[0]
        p = dict(errorCorrectionRate=1.0)
        return d, p, [family2_case(0), family2_case(0, seed=963), _damaged_frame("b2-bits", 5, d, p, 964, frame=F2_FRAME)]
    raise KeyError(name)


def all_cases():
    """Every frame tests/test_gpu_identify_damaged.py puts through the device, as (label, thunk)."""
    out = [(f"f1[{k}]", functools.partial(family1_case, k)) for k in range(len(FAMILY1))]
    out += [(f"f2[{k}]", functools.partial(family2_case, k)) for k in range(len(FAMILY2))]
    out += [(f"f3[{k}]", functools.partial(family3_case, k)) for k in range(len(FAMILY3))]
    out += [(f"f4[{k}]", functools.partial(family4_case, k)) for k in range(len(FAMILY4))]
    for g in BATCH_GROUPS:
        out += [(f"{g}[{i}]", functools.partial(lambda g, i: batch_group(g)[2][i], g, i)) for i in range(3)]
    return out
