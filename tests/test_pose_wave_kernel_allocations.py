"""The three kernels that run fid_pnp.h's wave-strided solve (pnp_wave_solve: k_map_pose plain and with its covariance tail,
k_map_pose_robust, k_charuco_pose) spill no vector register, stay one wave a SIMD (at most 512 allocated registers) and keep their
LDS layouts to the byte; k_map_pose and k_charuco_pose have no scratch, k_map_pose_robust at most the 160 B it had on its own
body.  Reads the kernel descriptors and notes of the built library through tools/occupancy.py, like
test_map_build_robust_kernel_allocations.py; needs the ROCm object tools, no GPU.

RECORDED (gfx950, -O3), allocated VGPRs for plumb-bob / rational / equidistant, on the shared body (before it, each kernel on its
own copy):
    k_map_pose, plain   368 / 408 / 400   (368 / 408 / 400)
    k_map_pose, cov     368 / 408 / 400   (384 / 416 / 400)
    k_map_pose_robust   424 / 456 / 464   (416 / 448 / 464)
    k_charuco_pose      360 / 400 / 392   (360 / 400 / 392)
LDS 63 760 B (MpLds), 64 144 B (RbLds), 25 872 B (ChPoseLds).  k_map_pose_robust keeps 160 B of scratch and parks 63 / 75 / 67
scalars in lanes of a vector register as before (the notes' sgpr_spill_count, printed below; no memory is involved)."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = (0, 1, 2)
MAP_POSE = tuple(f"k_map_pose<{m},false>" for m in MODELS) + tuple(f"k_map_pose<{m},true,double,fid_map_pose_cov*>" for m in MODELS)
ROBUST = tuple(f"k_map_pose_robust<{m}>" for m in MODELS)
CHARUCO = tuple(f"k_charuco_pose<{m}>" for m in MODELS)
LDS = dict([(n, 63760) for n in MAP_POSE] + [(n, 64144) for n in ROBUST] + [(n, 25872) for n in CHARUCO])
SCRATCH_MAX = dict([(n, 0) for n in MAP_POSE + CHARUCO] + [(n, 160) for n in ROBUST])
SGPR_PARKED = dict(zip(ROBUST, (63, 75, 67)))  # scalars parked in vector lanes; every other instantiation: none


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


def test_every_instantiation_is_in_the_library(sheet):
    assert set(LDS) <= set(sheet), sorted(n for n in sheet if n.startswith(("k_map_pose", "k_charuco_pose")))


def test_one_wave_a_simd_no_spills_the_lds_layouts_and_the_scratch_bounds(sheet):
    for name in LDS:
        k = sheet[name]
        print(f"{name}: vgpr_alloc {k['vgpr_alloc']}, sgpr {k['sgpr_count']}, lds {k['group_segment_fixed_size']}, scratch {k['private_segment_fixed_size']}, "
              f"vgpr spills {k['vgpr_spill_count']}, sgpr spills {k.get('sgpr_spill_count', 0)}")
        assert k["vgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_alloc"] <= 512, (name, k)
        assert k["group_segment_fixed_size"] == LDS[name], (name, k)
        assert k["private_segment_fixed_size"] <= SCRATCH_MAX[name], (name, k)
        assert k.get("sgpr_spill_count", 0) <= SGPR_PARKED.get(name, 0), (name, k)  # (the figures before the shared body: more is a regression)
