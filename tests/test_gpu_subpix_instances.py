"""k_subpix is instantiated per window bound (5, 7, 15): the same code over smaller arrays.  Windows up to 5 give under
k_subpix<5> the corners they give under k_subpix<7> (FID_SUBPIX_WIN7=1: the instantiation they ran on before) and the oracle's, on
markers in the frame's interior and on markers whose corner patches reach the frame's border; windows 6 and 7 still run
k_subpix<7>.  Run on the MI355X: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from fiducials_amd.detector import ArucoDetector
from fiducials_amd.dictionary import get_predefined_dictionary
from tail_frames import grid_frame, paste_frame
from test_gpu_parity import params_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240


def _dict():
    return get_predefined_dictionary("DICT_4X4_50")


def _frames(d):
    """Corners 3.6, 5.6 and 10.6 px from a border and markers in the interior.  With w the window, a corner's patch reaches
    w + 1.5 px and the pixels k_subpix keeps in LDS 2 w + 4 px from the corner: at 3.6 px the patch of windows 3 and 5 crosses the
    border (the replicated border) and window 1 has its patch inside but not its LDS copy (the uncached road), which is what 5.6 px
    is to window 3 and 10.6 px to window 5."""
    edge = paste_frame(d, [(3, 4, 4, 40), (5, 6, 120, 38), (7, W - 10 - 44, 60, 44), (9, 150, H - 6 - 36, 36), (11, 150, 90, 36)], W, H, 5)
    return np.stack([edge, grid_frame(d, 9, W, H, 41), grid_frame(d, 20, W, H, 42)])


@pytest.fixture(scope="module")
def frames():
    return _frames(_dict())


@pytest.mark.parametrize("win", [1, 3, 5])
def test_windows_up_to_5_equal_under_both_instantiations(frames, win, monkeypatch):
    d = _dict()
    p, op = params_pair(cornerRefinementWinSize=win)
    new = ArucoDetector(d, params=p, max_width=W, max_height=H, max_batch=3)
    monkeypatch.setenv("FID_SUBPIX_WIN7", "1")  # (read at fid_create)
    old = ArucoDetector(d, params=p, max_width=W, max_height=H, max_batch=3)
    monkeypatch.delenv("FID_SUBPIX_WIN7")
    try:
        moved = 0
        for f, img in enumerate(frames):
            a, b = new.detect_markers(img), old.detect_markers(img)
            pre = new.tap_presubpix()[0][:len(a[1])]["corners"].reshape(-1, 4, 2)
            oids, ocorners = oracle.detect(img, d, params=op)
            assert a[1].tolist() == b[1].tolist() == oids.tolist() and len(oids) == (5, 9, 20)[f]
            assert a[0].tobytes() == b[0].tobytes(), f
            assert np.array_equal(a[0], ocorners), f
            moved += int((a[0] != pre).any(axis=2).sum())
        assert moved >= 100  # (of 136 corners: the refinement did move them)
        ba, bb = new.detect_markers_batch(frames), old.detect_markers_batch(frames)
        for f in range(len(frames)):
            assert ba[f][0].tobytes() == bb[f][0].tobytes() and ba[f][1].tolist() == bb[f][1].tolist(), f
            assert np.array_equal(ba[f][0], new.detect_markers(frames[f])[0]), f
    finally:
        new.close()
        old.close()


_CHILD = """
import sys
import numpy as np
from fiducials_amd.detector import ArucoDetector, default_params
from fiducials_amd.dictionary import get_predefined_dictionary
from tail_frames import grid_frame
d = get_predefined_dictionary("DICT_4X4_50")
img = grid_frame(d, 9, 320, 240, 41)
for win in map(int, sys.argv[1:]):
    p = default_params()
    p.cornerRefinementWinSize = win
    det = ArucoDetector(d, params=p, max_width=320, max_height=240)
    assert len(det.detect_markers(img)[1]) == 9
    det.close()
"""


# (the launch log is opened once in a process, by its first launch: a process of its own per case)
@pytest.mark.parametrize("wins, force7, logged", [((1, 3, 5), False, {"k_subpix<5>"}), ((6, 7), False, {"k_subpix<7>"}),
                                                  ((1, 3, 5), True, {"k_subpix<7>"}), ((5, 7, 8), False, {"k_subpix<5>", "k_subpix<7>", "k_subpix<15>"})])
def test_the_window_chooses_the_instantiation(tmp_path, wins, force7, logged):
    log = tmp_path / "launches.txt"
    env = dict(os.environ, FID_LAUNCH_LOG=str(log), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env.pop("FID_SUBPIX_WIN7", None)
    if force7:
        env["FID_SUBPIX_WIN7"] = "1"
    subprocess.run([sys.executable, "-s", "-c", _CHILD] + [str(w) for w in wins], env=env, cwd=ROOT, check=True, timeout=120)
    lines = [ln.split() for ln in log.read_text().splitlines()]
    assert {ln[0] for ln in lines if ln[0].startswith("k_subpix")} == logged
    assert all(ln[1:] == ["64", "0"] for ln in lines if ln[0].startswith("k_subpix"))
