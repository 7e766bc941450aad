"""The point route of the calibration (fid_calib_points.hip) keeps nothing in scratch either: the kernels that read a view's rows
from the point table are in the built library, without scratch and without spills.  Reads the kernel descriptors like
test_calib_kernel_allocations.py (its `sheet`); needs the ROCm object tools, no GPU."""
from test_calib_kernel_allocations import sheet  # noqa: F401  (the fixture)

EXPECTED = ("k_calib_start_pts", "k_calib_init_pts", "k_calib_blocks_pts<0>", "k_calib_blocks_pts<1>", "k_calib_blocks_pts<2>", "k_calib_eval_pts<0>",
            "k_calib_eval_pts<1>", "k_calib_eval_pts<2>")


def test_every_kernel_of_the_point_route_is_in_the_library(sheet):  # noqa: F811
    names = sorted(n for n in sheet if n.startswith("k_calib_") and "_pts" in n)
    print(names)
    assert set(EXPECTED) == set(names), names


def test_no_scratch_no_spills(sheet):  # noqa: F811
    for name in EXPECTED:
        k = sheet[name]
        print(f"{name}: vgpr_alloc {k['vgpr_alloc']}, sgpr {k['sgpr_count']}, lds {k['group_segment_fixed_size']}, scratch {k['private_segment_fixed_size']}")
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
        assert k["vgpr_alloc"] <= 128, (name, k)
