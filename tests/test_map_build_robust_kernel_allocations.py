"""The trimmed map build's two kernels (fid_map_build.hip: k_build_place_score, k_build_obs_err) keep nothing in scratch and spill
nothing; their registers and LDS are recorded here.  Reads the kernel descriptors and notes of the built library through
tools/occupancy.py, like test_map_build_kernel_allocations.py; needs the ROCm object tools, no GPU.

RECORDED (gfx950, -O3): k_build_place_score<plumb-bob, rational, equidistant> 64 / 72 / 128 allocated VGPRs, 22 528 B of LDS (128
sixteen-bit counters a lane, 16 KB, and a lane's four map points, 6 KB): two waves a SIMD by LDS is the lower bound a CU never
meets, the grid being one wave a marker to place; k_build_obs_err 64 / 64 / 96 VGPRs, 928 B of LDS (the view's rotation).  No
kernel has scratch or spills a vector register.  The camera's 21 doubles and eight pointers fill the scalar registers of
k_build_place_score: its rational and equidistant instantiations park 12 and 2 scalars in lanes of a vector register (the notes'
sgpr_spill_count, printed below; no memory is involved), as test_map_build_kernel_allocations.py's conditions, which these are, allow."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = tuple(f"{k}<{m}>" for k in ("k_build_place_score", "k_build_obs_err") for m in (0, 1, 2))
SGPR_PARKED = {"k_build_place_score<1>": 12, "k_build_place_score<2>": 2}  # scalars parked in vector lanes; every other instantiation: none
LDS = {"k_build_place_score": 128 * 64 * 2 + 12 * 64 * 8, "k_build_obs_err": (36 + 80) * 8}


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


def test_both_kernels_are_in_the_library_for_every_camera_model(sheet):
    assert set(EXPECTED) <= set(sheet), sorted(n for n in sheet if n.startswith("k_build_"))


def test_no_scratch_no_spills_and_the_recorded_figures(sheet):
    for name in EXPECTED:
        k = sheet[name]
        print(f"{name}: vgpr_alloc {k['vgpr_alloc']}, sgpr {k['sgpr_count']}, lds {k['group_segment_fixed_size']}, scratch {k['private_segment_fixed_size']}, "
              f"vgpr spills {k['vgpr_spill_count']}, sgpr spills {k.get('sgpr_spill_count', 0)}")
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k.get("sgpr_spill_count", 0) <= SGPR_PARKED.get(name, 0), (name, k)  # (the recorded figures: more is a regression)
        assert k["vgpr_alloc"] <= 128, (name, k)
        assert k["group_segment_fixed_size"] == LDS[name.split("<")[0]], (name, k)
