"""MapBuilder::buildRobust (host/include/map_builder.hpp) through host/test/map_build_robust_test.cpp: the views of a
map_build_robust_cases case written out with the state the NumPy restatement gives every observation; the program builds through the
class, holds the states, rounds and stable to the file, and holds everything the class returns to the bytes of the C call."""
import os
import subprocess

import pytest

import map_build_robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "map_build_robust_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_map_build_robust_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_the_class_names_the_planted_observations_and_returns_the_c_call_s_bytes(tmp_path):
    c, ref = rc.case("moved"), rc.reference("moved")
    assert ref["kept"]
    o = ref["out"]
    k = c["k16"]
    f = c["fixed"][0]
    lines = [" ".join("%.17g" % v for v in list(k[:9]) + [c["fiducial_len"]]) + " 6 %.17g %d %d" % (rc.INLIER_PX, rc.MIN_VIEWS_PLACE, c["min_views"]),
             "%d %.17g " % (f["id"], f["len"]) + " ".join("%.17g" % v for v in list(f["R"].reshape(9)) + list(f["t"])), str(len(c["views"]))]
    for v, (corners, ids) in enumerate(c["views"]):
        lines.append(str(len(ids)))
        for p, (cr4, i) in enumerate(zip(corners, ids)):
            lines.append("%d " % i + " ".join("%.9g" % x for x in cr4.reshape(8)) + " %d" % o["obs_state"][v][p])
    lines.append("%d %d" % (o["rounds"], o["stable"]))
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([_build(), str(tmp_path / "views.txt"), os.path.join(ROOT, "fiducials_amd", "data")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
