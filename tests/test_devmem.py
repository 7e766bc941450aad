"""fid_devmem.h on the CPU: tests/devmem_main.cpp (the layout, the growing owner, "publish after success") built as a stand-alone
program with the address and undefined-behaviour sanitizers and run.  The header's two allocator calls are malloc / free there
(FID_DEVMEM_HOST_TEST), so a block the owner does not release is a leak the sanitizer reports."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_devmem_layout_and_owner_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/devmem_main.cpp")
    exe = str(tmp_path / "devmem_main")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: it runs the same whatever else the loader brings in)
           "-o", exe, os.path.join(HERE, "devmem_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "devmem ok", r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
