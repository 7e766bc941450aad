"""MapBuilder (host/include/map_builder.hpp) through host/test/map_build_test.cpp: the views of a map_build_cases case written out,
built through the class, saved as fiducial_slam's map file, read back by fid_map_load_file, set as the context's map, and
fid_map_pose_cam on some of the views gives those views' poses.  The built positions are held to the NumPy restatement's on the same
views at the parameter bar of tests/test_gpu_map_build.py."""
import os
import subprocess

import numpy as np
import pytest

import map_build_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "bin", "map_build_test")


def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return EXE


def test_map_build_test_builds_without_a_gpu():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_views_to_map_file_and_back(tmp_path):
    c, ref = mc.case("corner"), mc.reference("corner")
    assert ref["kept"], ref["gap"]
    best = ref["best"]
    t = max(10.0 * ref["gap"], 1e-9)
    bar = 2.0 * np.sqrt(2.0 * t * best["dof"]) * best["std"]
    k = c["k16"]
    f = c["fixed"][0]
    lines = [" ".join("%.17g" % v for v in list(k[:9]) + [c["fiducial_len"]]) + " 6",
             "%d %.17g " % (f["id"], f["len"]) + " ".join("%.17g" % v for v in list(f["R"].reshape(9)) + list(f["t"])), str(len(c["views"]))]
    for corners, ids in c["views"]:
        lines.append(str(len(ids)))
        for cr4, i in zip(corners, ids):
            lines.append("%d " % i + " ".join("%.9g" % v for v in cr4.reshape(8)))
    lines.append(str(len(best["mposes"])))
    for i, p in sorted(best["mposes"].items()):
        col = best["problem"].col[best["slot"][i]]
        lines.append("%d %.17g %.17g %.17g %.17g" % (i, p[3], p[4], p[5], bar[col + 3:col + 6].min()))
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([_build(), str(tmp_path / "views.txt"), os.path.join(ROOT, "fiducials_amd", "data"), str(tmp_path / "map.txt")],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    rows = [ln.split() for ln in (tmp_path / "map.txt").read_text().splitlines()]
    assert [int(x[0]) for x in rows] == sorted(int(e["id"]) for e in c["entries"])
    assert all(len(x) >= 10 for x in rows)  # every fiducial of the corner shares a view with another
