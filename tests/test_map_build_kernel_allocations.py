"""The map building kernels (fid_map_build.hip) keep nothing in scratch: rows, blocks, panels and right-hand sides that are indexed at
run time live in LDS.  Reads the kernel descriptors and notes of the built library through tools/occupancy.py, like
test_calib_kernel_allocations.py; needs the ROCm object tools, no GPU."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ("k_build_prep", "k_build_schur", "k_build_blocks<1>", "k_build_blocks<2>", "k_build_reduce", "k_build_panel", "k_build_update",
            "k_build_solve", "k_build_eval<1>", "k_build_eval<2>", "k_build_accept", "k_build_finish", "k_build_cov")


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


def test_every_map_building_kernel_is_in_the_library(sheet):
    names = sorted(n for n in sheet if n.startswith("k_build_"))
    print(names)
    assert set(EXPECTED) <= set(names), names


def test_no_scratch_no_spills(sheet):
    names = [n for n in sheet if n.startswith("k_build_")]
    assert names
    for name in names:
        k = sheet[name]
        print(f"{name}: vgpr_alloc {k['vgpr_alloc']}, sgpr {k['sgpr_count']}, lds {k['group_segment_fixed_size']}, scratch {k['private_segment_fixed_size']}")
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_alloc"] <= 128, (name, k)
