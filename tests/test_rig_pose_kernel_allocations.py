"""k_rig_pose (fid_rig_pose.hip: the gather over a rig's cameras, pnp_wave_solve for each of the three models behind a switch on the
start camera's, the joint Levenberg-Marquardt solve and the covariance tail, one instantiation) spills no vector register, stays
one wave a SIMD (at most 512 allocated registers) and keeps its LDS layout to the byte.  Reads the kernel descriptor and notes of
the built library through tools/occupancy.py, like test_pose_wave_kernel_allocations.py; needs the ROCm object tools, no GPU.

RECORDED (gfx950, -O3): 424 allocated VGPRs, LDS 42 072 B (RgLds), no scratch, 4 scalars parked in lanes of a vector register (the
notes' sgpr_spill_count, printed below; no memory is involved)."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "k_rig_pose"
LDS = 42072
RECORDED_SCRATCH = 0
SGPR_PARKED = 4


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
    return {occ.short(dm.get(m, m)).replace(" ", ""): dict(meta, vgpr_alloc=alloc[m]) for m, meta in notes.items()}


def test_the_kernel_is_in_the_library(sheet):
    assert NAME in sheet, sorted(n for n in sheet if "rig" in n)


def test_one_wave_a_simd_no_spills_the_lds_layout_and_the_scratch(sheet):
    k = sheet[NAME]
    print(f"{NAME}: vgpr_alloc {k['vgpr_alloc']}, sgpr {k['sgpr_count']}, lds {k['group_segment_fixed_size']}, scratch {k['private_segment_fixed_size']}, "
          f"vgpr spills {k['vgpr_spill_count']}, sgpr spills {k.get('sgpr_spill_count', 0)}")
    assert k["vgpr_spill_count"] == 0, k
    assert k["vgpr_alloc"] <= 512, k
    assert k["group_segment_fixed_size"] == LDS, k
    assert k["private_segment_fixed_size"] == RECORDED_SCRATCH, k
    assert k.get("sgpr_spill_count", 0) <= SGPR_PARKED, k
