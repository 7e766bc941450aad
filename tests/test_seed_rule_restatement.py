"""The tracing-seed rule (fid_device.h: seed_state, seed_empty_dir; the HYB blocks of k_find_starts and k_find_seeds) restated in
NumPy, so that a test can say how many seeds a mask has without asking either kernel: a seed is a state (pixel, d) whose pixel
is foreground and lies on a grid line that d may enter (a column x = 0 mod G with a horizontal component in d, a row y = 0 mod G
with a vertical one), whose neighbour in direction d is foreground and whose neighbour in direction seed_empty_dir(d) is
background.  Here the vectorised restatement (seed_map, used by tests/test_gpu_seed_kernel.py) is checked against the rule
evaluated pixel by pixel, state by state."""
import numpy as np

# directions as everywhere in the library: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE (y grows downwards)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)
SEED_DIRS_COL = 0xBB  # directions with a horizontal component
SEED_DIRS_ROW = 0xEE  # directions with a vertical component


def seed_empty_dir(d):
    return (d + (1 if d & 1 else 2)) & 7


def seed_map(mask, grid):
    """mask: (H, W) bool / 0-255 foreground; grid: spacing G.  Returns bool (8, H, W): state (x, y, d) is a seed."""
    m = np.asarray(mask) > 0
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = m
    nb = [p[1 + DY[d]:1 + DY[d] + h, 1 + DX[d]:1 + DX[d] + w] for d in range(8)]
    on_col = (np.arange(w) % grid == 0)[None, :]
    on_row = (np.arange(h) % grid == 0)[:, None]
    out = np.zeros((8, h, w), bool)
    for d in range(8):
        line = np.zeros((h, w), bool)
        if (SEED_DIRS_COL >> d) & 1:
            line |= on_col
        if (SEED_DIRS_ROW >> d) & 1:
            line |= on_row
        out[d] = m & nb[d] & ~nb[seed_empty_dir(d)] & line
    return out


def seed_count(mask, grid):
    return int(seed_map(mask, grid).sum())


def brute_force_seeds(mask, grid):
    m = np.asarray(mask) > 0
    h, w = m.shape

    def fg(x, y):
        return 0 <= x < w and 0 <= y < h and bool(m[y, x])

    seeds = set()
    for y in range(h):
        for x in range(w):
            if not m[y, x]:
                continue
            for d in range(8):
                state = (x % grid == 0 and (SEED_DIRS_COL >> d) & 1) or (y % grid == 0 and (SEED_DIRS_ROW >> d) & 1)
                e = seed_empty_dir(d)
                if state and fg(x + DX[d], y + DY[d]) and not fg(x + DX[e], y + DY[e]):
                    seeds.add((x, y, d))
    return seeds


def test_restatement_equals_the_rule_pixel_by_pixel():
    rng = np.random.default_rng(20)
    total = 0
    for density in (0.15, 0.5, 0.85):
        mask = rng.random((80, 96)) < density
        mask[32, 10:40] = True   # a run along a grid row, a run along a grid column, a block on a crossing
        mask[40:70, 64] = True
        mask[60:68, 28:36] = True
        got = seed_map(mask, 32)
        want = brute_force_seeds(mask, 32)
        assert {(int(x), int(y), int(d)) for d, y, x in zip(*np.nonzero(got))} == want
        assert seed_count(mask, 32) == len(want)
        total += len(want)
    assert total > 500  # (the masks do have seeds, on rows, columns and crossings)
    on = np.nonzero(seed_map(np.ones((80, 96), bool), 32))
    assert len(on[0]) > 0 and all((x % 32 == 0) or (y % 32 == 0) for _, y, x in zip(*on))  # (a full mask: seeds on the image border's lines only)


def test_empty_dir_is_the_neighbour_right_of_travel():
    assert [seed_empty_dir(d) for d in range(8)] == [2, 2, 4, 4, 6, 6, 0, 0]
