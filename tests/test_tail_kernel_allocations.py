"""What the built library allocates for k_subpix<5>, the instantiation the node's cornerRefinementWinSize (5) runs on: its static
LDS is what lets more workgroups onto a CU than k_subpix<7> (11 928 B: 13 a CU), so it is held below 7 KB (23 a CU by LDS: the
registers bind first), without scratch memory or spills, and at no more registers than k_subpix<7>.  Reads descriptors and notes
only; needs the ROCm object tools, no GPU."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sheet():
    spec = importlib.util.spec_from_file_location("occupancy", os.path.join(ROOT, "tools", "occupancy.py"))
    occ = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(occ)
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


def test_subpix_5_lds_and_registers(sheet):
    k5, k7 = sheet["k_subpix<5>"], sheet["k_subpix<7>"]
    print(f"k_subpix<5>: {k5['group_segment_fixed_size']} B of LDS, {k5['vgpr_alloc']} registers; k_subpix<7>: "
          f"{k7['group_segment_fixed_size']} B, {k7['vgpr_alloc']}")
    assert k5["group_segment_fixed_size"] < 7 * 1024, k5
    assert k5["private_segment_fixed_size"] == 0 and k5["vgpr_spill_count"] == 0, k5
    assert k5["vgpr_alloc"] <= k7["vgpr_alloc"], (k5, k7)
