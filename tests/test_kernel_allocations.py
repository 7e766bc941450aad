"""Registers a wave is ALLOCATED, from the kernel descriptors of the built library (round 9).

The hardware sizes a wave's register allocation by the descriptor (<kernel>.kd: compute_pgm_rsrc1, granule 8), not by the notes'
.vgpr_count.  For a kernel with a large static LDS footprint the compiler pads the descriptor up to the floor of the occupancy the
LDS allows (k_seed_walk used 116 registers and was allocated 176): registers that keep the other sub-batch's kernels off the CU for
nothing.  The walkers declare a workgroup upper bound that takes the padding away (fid_kernels.hip, WALKER_WG_ATTR); this test holds
the descriptors to what the kernels use.  Reads descriptors and notes only; needs the ROCm object tools, no GPU."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WALKERS = ("k_seed_walk", "k_walk_full<0>", "k_walk_full<2>")
UNPADDED = WALKERS + ("k_seg_cycles<48u>",)
THRESHOLD = ("k_threshold_stream<3,4,13,3,false>", "k_threshold_stream<3,4,13,3,true>", "k_threshold_stream<3,4,13,5,false>",
             "k_threshold_stream<3,4,13,5,true>")


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
    out = {}
    for mangled, meta in notes.items():
        out[occ.short(dm.get(mangled, mangled))] = dict(meta, vgpr_alloc=alloc[mangled])
    return out


def _ceil8(n):
    return max(8, -(-n // 8) * 8)


@pytest.mark.parametrize("name", UNPADDED)
def test_descriptor_allocation_is_what_the_kernel_uses(sheet, name):
    k = sheet[name]
    # (.vgpr_count is the unified count: architectural registers, aligned, plus accumulation registers)
    used = max(k["vgpr_count"], k["agpr_count"])
    print(f"{name}: uses {used}, descriptor allocates {k['vgpr_alloc']}")
    assert k["vgpr_alloc"] == _ceil8(used), (name, k)


def test_walkers_keep_their_static_lds_and_fit_beside_three_threshold_workgroups(sheet):
    occ = _tool()
    thr = sheet[THRESHOLD[0]]
    host = {"vgpr": thr["vgpr_alloc"], "agpr": 0, "sgpr": thr["sgpr_count"], "lds": 31104, "block": 256}
    for name, block in (("k_seed_walk", 128), ("k_walk_full<2>", 256)):
        k = sheet[name]
        assert k["group_segment_fixed_size"] == 34816, name
        guest = {"vgpr": k["vgpr_alloc"], "agpr": 0, "sgpr": k["sgpr_count"], "lds": 34816, "block": block}
        assert occ.fits_beside(host, 3, guest)["workgroups"] >= 1, name


@pytest.mark.parametrize("name", UNPADDED + THRESHOLD)
def test_no_scratch_no_spills(sheet, name):
    k = sheet[name]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
    assert k["vgpr_alloc"] <= 128, (name, k)  # four waves per SIMD at the least
