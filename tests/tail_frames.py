"""Small synthetic frames with a marker count and marker places that are known by construction, for the tests of the candidate
tail's work order (test_gpu_tail_order.py) and of the k_subpix instantiations (test_gpu_subpix_instances.py): upright markers
pasted on a light sheet, blurred and with noise, so that cornerSubPix moves every corner.  No GPU here."""
import numpy as np

from fiducials_amd.dictionary import draw_marker
from fiducials_amd.synth import _blur


def paste_frame(d, places, width, height, seed):
    """places: (id, x, y, side) per marker, the top-left corner and the side in pixels.  A marker may come as close to the frame's
    border as minDistanceToBorder allows; the light sheet is its quiet zone."""
    rng = np.random.default_rng(seed)
    img = np.full((height, width), 205.0, np.float32)
    for mid, x, y, side in places:
        m = draw_marker(d, int(mid), int(side), 1)
        img[y:y + side, x:x + side] = np.where(m > 0, 230.0, 25.0)
    img = _blur(img, 0.8) + rng.normal(0.0, 2.0, size=img.shape).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def grid_frame(d, n, width, height, seed, pitch=50):
    """n markers on a pitch x pitch grid in a random choice of its cells, sides of 28 ... 34 px, places jittered by up to 3 px."""
    rng = np.random.default_rng(1000 + seed)
    cols, rows = (width - 10) // pitch, (height - 10) // pitch
    assert n <= cols * rows, (n, cols, rows)
    cells = rng.permutation(cols * rows)[:n]
    ids = rng.permutation(d.n_markers)[:n]
    places = []
    for cell, mid in zip(cells, ids):
        side = int(rng.integers(28, 35))
        x = 8 + (cell % cols) * pitch + int(rng.integers(0, 4))
        y = 8 + (cell // cols) * pitch + int(rng.integers(0, 4))
        places.append((int(mid), x, y, side))
    return paste_frame(d, places, width, height, seed)
