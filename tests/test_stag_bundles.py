"""Tag bundles on the STag path, the parts that need no device: the layout loader (stag_ros/load_yaml_tags.h), the board scenes the
GPU tests use (the reference's own detector must find every tag of them), and the oracle's pose on them."""
import numpy as np
import pytest

import stag_bundle_cases as bc
from fiducials_amd import _lib, stag as fstag

BLOCK = """\
# two bundles and two standalone tags, block style
tags:
  - id: 40
    frame: tag_40
    corners:
      - [-0.04, -0.04, 0.0]
      - [0.04, -0.04, 0.0]
      - [0.04, 0.04, 0.0]
  - id: 41
    frame: "tag 41"   # a quoted name
    corners:
      - - -0.1
        - -0.1
        - 0
      - - 0.1
        - -0.1
        - 0
      - - 0.1
        - 0.1
        - 0
bundles:
  - frame: plate
    tags:
      - id: 0
        corners:
          - [0.0, 0.0, 0.0]
          - [0.08, 0.0, 0.0]
          - [0.08, 0.08, 0.0]
      - id: 1
        corners:
          - [0.1, 0.0, 0.0]
          - [0.18, 0.0, 0.0]
          - [0.18, 0.08, 0.0]
  - frame: tool
    tags:
    - id: 7
      corners: [[0, 0, 0.08], [0, 0, 0], [0, 0.08, 0]]
    - id: 8
      corners: [[0.02, 0, 0], [0.10, 0, 0], [0.10, 0.08, 0]]
    - id: 9
      corners: [[1.5e-1, 0, 0], [2.3e-1, 0, 0], [2.3e-1, 0.08, 0.001]]
"""

FLOW = """\
tags: [{id: 40, frame: tag_40, corners: [[-0.04, -0.04, 0.0], [0.04, -0.04, 0.0], [0.04, 0.04, 0.0]]},
       {id: 41, frame: 'tag 41', corners: [[-0.1, -0.1, 0], [0.1, -0.1, 0], [0.1, 0.1, 0]]}]
bundles: [{frame: plate, tags: [{id: 0, corners: [[0.0, 0.0, 0.0], [0.08, 0.0, 0.0], [0.08, 0.08, 0.0]]},
                                {id: 1, corners: [[0.1, 0.0, 0.0], [0.18, 0.0, 0.0], [0.18, 0.08, 0.0]]}]},
          {frame: tool, tags: [{id: 7, corners: [[0, 0, 0.08], [0, 0, 0], [0, 0.08, 0]]},
                               {id: 8, corners: [[0.02, 0, 0], [0.10, 0, 0], [0.10, 0.08, 0]]},
                               {id: 9, corners: [[1.5e-1, 0, 0], [2.3e-1, 0, 0], [2.3e-1, 0.08, 0.001]]}]}]
"""

THREE = {40: [[-0.04, -0.04, 0.0], [0.04, -0.04, 0.0], [0.04, 0.04, 0.0]], 41: [[-0.1, -0.1, 0], [0.1, -0.1, 0], [0.1, 0.1, 0]],
         0: [[0.0, 0.0, 0.0], [0.08, 0.0, 0.0], [0.08, 0.08, 0.0]], 1: [[0.1, 0.0, 0.0], [0.18, 0.0, 0.0], [0.18, 0.08, 0.0]],
         7: [[0, 0, 0.08], [0, 0, 0], [0, 0.08, 0]], 8: [[0.02, 0, 0], [0.10, 0, 0], [0.10, 0.08, 0]],
         9: [[0.15, 0, 0], [0.23, 0, 0], [0.23, 0.08, 0.001]]}


def _load(tmp_path, text, name="layout.yaml"):
    p = tmp_path / name
    p.write_text(text)
    return fstag.load_layout(str(p))


def test_loader_block_and_flow_style_give_the_same_layout(tmp_path):
    a, b = _load(tmp_path, BLOCK, "block.yaml"), _load(tmp_path, FLOW, "flow.yaml")
    assert a.tags.tobytes() == b.tags.tobytes() and a.frames == b.frames and a.standalone.tolist() == b.standalone.tolist()
    # bundles first, in file order, then the standalone tags; tags ordered by bundle
    assert a.frames == ["plate", "tool", "tag_40", "tag 41"]
    assert a.standalone.tolist() == [False, False, True, True]
    assert a.tags["id"].tolist() == [0, 1, 7, 8, 9, 40, 41]
    assert a.tags["bundle"].tolist() == [0, 0, 1, 1, 1, 2, 3]
    for t in a.tags:
        c = np.array(THREE[int(t["id"])], float)
        assert np.array_equal(t["corners"][:3], c)
        # load_yaml_tags.h:28-30
        assert np.array_equal(t["center"], (c[2] + c[0]) / 2)
        assert np.array_equal(t["corners"][3], c[0] + (c[2] - c[1]))


def test_tag_from_three_corners_is_the_loaders_arithmetic():
    rng = np.random.default_rng(5)
    for _ in range(20):
        c = rng.normal(size=(3, 3))
        t = fstag.tag_from_three_corners(3, 2, c[0], c[1], c[2])
        assert t["id"] == 3 and t["bundle"] == 2
        assert np.array_equal(t["center"], (c[2] + c[0]) / 2) and np.array_equal(t["corners"][3], c[0] + (c[2] - c[1]))


@pytest.mark.parametrize("what,text", [
    ("truncated flow", FLOW[:FLOW.index("{id: 8")]),
    ("truncated block", BLOCK[:BLOCK.index("          - [0.08, 0.08, 0.0]")]),
    ("corner with two numbers", BLOCK.replace("[0.18, 0.0, 0.0]", "[0.18, 0.0]")),
    ("missing id", BLOCK.replace("      - id: 1\n        corners:", "      - corners:")),
    ("missing id in flow", FLOW.replace("{id: 8, ", "{")),
    ("duplicate id", BLOCK.replace("id: 41", "id: 7")),
    ("not a number", BLOCK.replace("[0.1, 0.0, 0.0]", "[0.1, abc, 0.0]")),
    ("empty", "# nothing\n"),
])
def test_loader_refuses_malformed_files_with_a_message(tmp_path, what, text):
    with pytest.raises(fstag.FidError) as e:
        _load(tmp_path, text)
    assert e.value.status == _lib.FID_E_INVALID_ARG, what
    assert "layout.yaml" in str(e.value) and len(_lib.load().fid_stag_layout_last_error()) > 10
    # never a half-read layout: the C call leaves both counts at 0
    import ctypes as C
    nt, nb = C.c_int32(-1), C.c_int32(-1)
    tags = np.zeros(64, fstag.TAG_DTYPE)
    rc = _lib.load().fid_stag_layout_load_file(str(tmp_path / "layout.yaml").encode(), tags.ctypes.data, 64, C.byref(nt), C.byref(nb), None, None, 0)
    assert rc == _lib.FID_E_INVALID_ARG and nt.value == 0 and nb.value == 0 and not tags.tobytes().strip(b"\0")


def test_loader_reports_what_a_small_buffer_needs(tmp_path):
    import ctypes as C
    p = tmp_path / "layout.yaml"
    p.write_text(BLOCK)
    nt, nb = C.c_int32(0), C.c_int32(0)
    tags = np.zeros(2, fstag.TAG_DTYPE)
    rc = _lib.load().fid_stag_layout_load_file(str(p).encode(), tags.ctypes.data, 2, C.byref(nt), C.byref(nb), None, None, 0)
    assert rc == _lib.FID_E_CAPACITY and (nt.value, nb.value) == (7, 4)
    assert _lib.load().fid_stag_layout_load_file(b"/nonexistent/layout.yaml", tags.ctypes.data, 2, C.byref(nt), C.byref(nb), None, None, 0) == _lib.FID_E_INVALID_ARG


def _ref_or_skip():
    from oracle import stag_ref
    if not stag_ref.available():
        pytest.skip("oracle/_ref/libstag_ref.so not built (needs /root/reference at build time)")
    return stag_ref


@pytest.mark.parametrize("board,pose", bc.all_scenes())
def test_board_scenes_are_detectable_by_the_reference_alone(board, pose):
    """Every tag of every scene is found by the reference's own Stag::detectMarkers, and tag 0's first corner is the texture's top-left
    one (the order fid_stag_tag.corners is declared in).  The bound on that corner is 1 px: a corner order turned by one place is off
    by a tag's side (70 px and more here), and the reference's corners scatter around the rendered ones by its own line fits on
    sigma-2 noise -- 0.06 ... 0.37 px over the 36 tags of the nine scenes, with one at 0.75 px (hd21_3x2, pose 0, tag 0; 0.04 px on
    the same scene without noise)."""
    stag_ref = _ref_or_skip()
    hd, ids, _, _ = bc.BOARDS[board]
    fr = bc.scene(board, pose)
    ref = stag_ref.detect_markers(fr.image, hd, 7 if hd == 21 else 2)
    assert sorted(ref[:, 0].astype(int).tolist()) == list(ids), (board, pose, ref[:, 0])
    k = ref[:, 0].astype(int).tolist().index(0)
    d = float(np.linalg.norm(ref[k, 1:3] - fr.corners_image[0, 0]))
    print(board, pose, "corner 0 of tag 0:", round(d, 3), "px from the texture's top-left corner")
    assert d < 1.0


@pytest.mark.parametrize("board,pose", bc.hd21_scenes())
def test_oracle_pose_on_the_board_scenes(board, pose):
    """cv::solvePnP restated, on the reference's detections and the board geometry, against the rendered pose: translation within
    2 % of |t| (the bar of test_gpu_stag.py's marker pose) and board normal within 1 degree from the whole board; from one tag the
    translation bound holds as well, its normal is printed (a single fronto-parallel 83 px tag under sigma-2 noise: 1.04 degrees on
    hd21_3x2 pose 0 -- the conditioning a bundle is there to improve)."""
    import oracle
    from fiducials_amd import synth
    stag_ref = _ref_or_skip()
    fr = bc.scene(board, pose)
    m = bc.ref_markers_as_dtype(stag_ref.detect_markers(fr.image, 21, 7))
    for sel in (m, m[:1]):
        r, t = oracle.solve_pnp_points(bc.K, np.zeros(5), bc.board_points(fr, sel["id"]), bc.marker_points(sel))
        terr = np.linalg.norm(t - fr.tvec) / np.linalg.norm(fr.tvec)
        nerr = bc.angle_deg(synth._rodrigues(r)[:, 2], fr.R[:, 2])
        print(board, pose, len(sel), "tag(s): translation error %.4f %% of |t|, normal %.3f degrees" % (100 * terr, nerr))
        assert terr < 0.02, (len(sel), t, fr.tvec)
        if len(sel) == len(m):
            assert nerr < 1.0
