"""Every STag kernel is one functor (struct k_stag_X_fn: launch bound, parameter list and body, once) under two generic entries,
k_stag_frame<k_stag_X_fn, A...> (a frame at a time) and k_stag_batch<k_stag_X_fn> (a group of frames, fid_stag_batch.h).  Before, each
kernel was a body function behind a named kernel and a functor.  For every functor both instantiations must be in the built library,
and neither may cost more than the same kernel did in the build of the commit before the change: no more allocated VGPRs, the LDS
equal to the byte, no scratch where there was none (nor more of it), no vector-register spill, no more scalars parked in vector
lanes.  Reads the kernel descriptors and notes of the built library through tools/occupancy.py, like
test_pose_wave_kernel_allocations.py; needs the ROCm object tools, no GPU.

PARENT is that build's sheet (gfx950, -O3), generated with tools/occupancy.py's readers from a library built from the parent
commit, the frame form under the name its kernel had then (tools/occupancy.py short() gives k_stag_frame<k_stag_X_fn, ...> the same
name).  k_stag_memset and k_stag_memcpy have a group form only: nothing ever launched their named kernels (a frame on its own uses
hipMemsetAsync / hipMemcpyAsync, fid_stag_batch.h), so no frame entry is instantiated for them.  The two _cov pose kernels are
never recorded and stay plain kernels over the shared body; they are held to the same figures."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (allocated VGPRs, static LDS bytes, scratch bytes, vector-register spills, scalars parked in vector lanes)
PARENT = {
    "k_stag_anchors": (16, 0, 0, 0, 0),
    "k_stag_anchors[g]": (16, 0, 0, 0, 0),
    "k_stag_bandscan": (56, 0, 0, 0, 0),
    "k_stag_bandscan[g]": (56, 0, 0, 0, 0),
    "k_stag_bandsum": (8, 0, 0, 0, 0),
    "k_stag_bandsum[g]": (8, 0, 0, 0, 0),
    "k_stag_batch<k_stag_bundle_pose_fn<0>>": (256, 5856, 0, 0, 0),
    "k_stag_batch<k_stag_bundle_pose_fn<1>>": (296, 5856, 0, 0, 2),
    "k_stag_batch<k_stag_bundle_pose_fn<2>>": (304, 5856, 0, 0, 0),
    "k_stag_batch<k_stag_pose_fn<0>>": (232, 0, 208, 0, 0),
    "k_stag_batch<k_stag_pose_fn<1>>": (272, 0, 208, 0, 0),
    "k_stag_batch<k_stag_pose_fn<2>>": (280, 0, 208, 0, 0),
    "k_stag_bundle_pose<0>": (256, 5856, 0, 0, 0),
    "k_stag_bundle_pose<1>": (296, 5856, 0, 0, 0),
    "k_stag_bundle_pose<2>": (304, 5856, 0, 0, 0),
    "k_stag_bundle_pose_cov<0>": (256, 5856, 0, 0, 0),
    "k_stag_bundle_pose_cov<1>": (296, 5856, 0, 0, 5),
    "k_stag_bundle_pose_cov<2>": (304, 5856, 0, 0, 0),
    "k_stag_ccl_border": (24, 0, 0, 0, 0),
    "k_stag_ccl_border[g]": (24, 0, 0, 0, 0),
    "k_stag_ccl_flatten": (16, 896, 0, 0, 0),
    "k_stag_ccl_flatten[g]": (16, 896, 0, 0, 6),
    "k_stag_ccl_tile": (24, 4352, 0, 0, 0),
    "k_stag_ccl_tile[g]": (24, 4352, 0, 0, 0),
    "k_stag_comp_alloc": (40, 0, 0, 0, 0),
    "k_stag_comp_alloc[g]": (40, 0, 0, 0, 0),
    "k_stag_comp_fill": (16, 0, 0, 0, 0),
    "k_stag_comp_fill[g]": (16, 0, 0, 0, 0),
    "k_stag_comp_sort": (88, 32768, 0, 0, 0),
    "k_stag_comp_sort[g]": (88, 32768, 0, 0, 0),
    "k_stag_comp_sort_big": (48, 0, 0, 0, 0),
    "k_stag_comp_sort_big[g]": (48, 0, 0, 0, 0),
    "k_stag_comp_tilemax": (8, 0, 0, 0, 0),
    "k_stag_comp_tilemax[g]": (8, 0, 0, 0, 0),
    "k_stag_compact_lines": (24, 0, 0, 0, 0),
    "k_stag_compact_lines[g]": (24, 0, 0, 0, 0),
    "k_stag_decode": (112, 4096, 104, 0, 0),
    "k_stag_decode[g]": (112, 4096, 104, 0, 0),
    "k_stag_dedup": (56, 0, 0, 0, 0),
    "k_stag_dedup[g]": (56, 0, 0, 0, 0),
    "k_stag_extract": (16, 0, 0, 0, 0),
    "k_stag_extract[g]": (16, 0, 0, 0, 0),
    "k_stag_fills": (8, 0, 0, 0, 0),
    "k_stag_fills[g]": (8, 0, 0, 0, 0),
    "k_stag_gather_lines": (24, 0, 0, 0, 0),
    "k_stag_gather_lines[g]": (24, 0, 0, 0, 0),
    "k_stag_gather_quads": (32, 0, 0, 0, 0),
    "k_stag_gather_quads[g]": (32, 0, 0, 0, 0),
    "k_stag_ingest": (40, 0, 0, 0, 0),
    "k_stag_ingest[g]": (40, 0, 0, 0, 0),
    "k_stag_line_ranges": (8, 0, 0, 0, 0),
    "k_stag_line_ranges[g]": (8, 0, 0, 0, 0),
    "k_stag_memcpy[g]": (16, 0, 0, 0, 0),
    "k_stag_memset[g]": (16, 0, 0, 0, 0),
    "k_stag_next_above": (80, 64, 0, 0, 23),
    "k_stag_next_above[g]": (80, 64, 0, 0, 26),
    "k_stag_place": (80, 24576, 0, 0, 0),
    "k_stag_place[g]": (80, 24576, 0, 0, 0),
    "k_stag_pose<0>": (232, 0, 208, 0, 0),
    "k_stag_pose<1>": (272, 0, 208, 0, 0),
    "k_stag_pose<2>": (280, 0, 208, 0, 0),
    "k_stag_pose_cov<0>": (232, 0, 208, 0, 0),
    "k_stag_pose_cov<1>": (272, 0, 208, 0, 0),
    "k_stag_pose_cov<2>": (280, 0, 208, 0, 0),
    "k_stag_quads": (80, 0, 0, 0, 0),
    "k_stag_quads[g]": (80, 0, 0, 0, 0),
    "k_stag_refine": (240, 1272, 1232, 0, 0),
    "k_stag_refine[g]": (240, 1272, 1232, 0, 0),
    "k_stag_route_extract": (264, 131136, 0, 0, 0),
    "k_stag_route_extract[g]": (264, 131136, 0, 0, 0),
    "k_stag_route_extract_big": (264, 32800, 0, 0, 0),
    "k_stag_route_extract_big[g]": (264, 32800, 0, 0, 0),
    "k_stag_route_extract_small": (104, 32832, 0, 0, 0),
    "k_stag_route_extract_small[g]": (104, 32832, 0, 0, 0),
    "k_stag_route_gather": (40, 0, 0, 0, 0),
    "k_stag_route_gather[g]": (40, 0, 0, 0, 0),
    "k_stag_route_seq": (24, 0, 0, 0, 0),
    "k_stag_route_seq[g]": (24, 0, 0, 0, 4),
    "k_stag_route_walk": (104, 2052, 0, 0, 43),
    "k_stag_route_walk[g]": (104, 2052, 0, 0, 57),
    "k_stag_scan": (16, 2048, 0, 0, 0),
    "k_stag_scan[g]": (16, 2048, 0, 0, 0),
    "k_stag_scan_counts": (72, 64, 0, 0, 0),
    "k_stag_scan_counts[g]": (72, 64, 0, 0, 0),
    "k_stag_scan_counts_n": (72, 32832, 0, 0, 0),
    "k_stag_scan_counts_n[g]": (72, 32832, 0, 0, 0),
    "k_stag_smooth3_prewitt": (24, 11528, 0, 0, 0),
    "k_stag_smooth3_prewitt[g]": (24, 11528, 0, 0, 0),
    "k_stag_smooth_grad": (24, 5800, 0, 0, 0),
    "k_stag_smooth_grad[g]": (32, 5800, 0, 0, 0),
    "k_stag_spec_guard": (8, 0, 0, 0, 0),
    "k_stag_spec_guard[g]": (8, 0, 184, 0, 0),
    "k_stag_split_lines": (88, 0, 0, 0, 0),
    "k_stag_split_lines[g]": (88, 0, 0, 0, 0),
    "k_stag_test_segments": (48, 0, 0, 0, 0),
    "k_stag_test_segments[g]": (48, 0, 0, 0, 0),
    "k_stag_valid_prob": (72, 2048, 0, 0, 0),
    "k_stag_valid_prob[g]": (72, 2048, 0, 0, 0),
    "k_stag_validate_lines": (72, 0, 0, 0, 0),
    "k_stag_validate_lines[g]": (72, 0, 0, 0, 0),
}
GROUP_ONLY = ("k_stag_memset", "k_stag_memcpy")


def _tool():
    spec = importlib.util.spec_from_file_location("occupancy", os.path.join(ROOT, "tools", "occupancy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def sheet():
    occ = _tool()
    tools = [os.path.join(occ.LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools) or shutil.which("c++filt") is None:
        pytest.skip("ROCm object tools (llvm-objcopy, clang-offload-bundler, llvm-readelf) or c++filt not installed")
    lib = os.path.join(ROOT, "fiducials_amd", "lib", "libfid_amd.so")
    with tempfile.TemporaryDirectory() as td:
        co = occ.code_object(lib, td)
        notes = occ.read_notes(co)
        alloc = occ.read_descriptors(co)
    dm = occ.demangle(list(notes))
    return {occ.short(dm.get(m, m)): dict(meta, vgpr_alloc=alloc[m]) for m, meta in notes.items()}


def test_the_table_holds_both_forms_of_every_functor():
    # 37 kernels with a body of their own + the three route_extract footprints + memset / memcpy, pose and bundle pose per camera model
    frame = [n for n in PARENT if not n.endswith("[g]") and not n.startswith("k_stag_batch<") and "_cov<" not in n]
    assert len(frame) == 40 + 2 * 3
    for n in frame:
        g = f"k_stag_batch<{n.replace('<', '_fn<')}>" if "<" in n else n + "[g]"
        assert g in PARENT, (n, g)
    assert all(n + "[g]" in PARENT and n not in PARENT for n in GROUP_ONLY)
    assert len(PARENT) == 2 * len(frame) + len(GROUP_ONLY) + 6


def test_both_instantiations_of_every_functor_are_in_the_library(sheet):
    missing = sorted(set(PARENT) - set(sheet))
    assert not missing, (missing, sorted(n for n in sheet if "k_stag_" in n))


def test_no_kernel_costs_more_than_before(sheet):
    for name, (vgpr, lds, scratch, vspill, sspill) in PARENT.items():
        k = sheet[name]
        print(f"{name}: vgpr_alloc {k['vgpr_alloc']} ({vgpr}), lds {k['group_segment_fixed_size']} ({lds}), scratch {k['private_segment_fixed_size']} ({scratch}), "
              f"vgpr spills {k['vgpr_spill_count']} ({vspill}), sgpr spills {k.get('sgpr_spill_count', 0)} ({sspill})")
        assert k["vgpr_alloc"] <= vgpr, (name, k)
        assert k["group_segment_fixed_size"] == lds, (name, k)
        assert k["private_segment_fixed_size"] <= scratch, (name, k)
        assert k["vgpr_spill_count"] <= vspill, (name, k)
        assert k.get("sgpr_spill_count", 0) <= sspill, (name, k)
