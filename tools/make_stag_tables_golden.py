#!/usr/bin/env python3
"""tests/golden/stag_host_tables.npz: the reference's own host tables for the image sizes tests/test_oracle_stag_ref.py checks,
so that the product's fid_stag_host_tables is checked where oracle/_ref cannot be built.  Per size WxH: NFALUT (<WxH>_lut),
ComputeMinLineLength (<WxH>_mll), Stag::fillCodeLocations (<WxH>_locs) and, for every segment length n the product's table
covers past the LUT, the least k with nfa(n, k) >= 0, or n + 1 where there is none (<WxH>_kmin, indexed by n - len(lut)).
Run where oracle/_ref is built (needs /root/reference at build time)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fiducials_amd import _lib  # noqa: E402
from oracle import stag_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "stag_host_tables.npz")
SIZES = [(1920, 1080), (640, 480), (320, 240), (160, 120)]


def least_k(n, w, h):
    """nfa(n, k) falls as k grows: the least valid k by bisection over [0, n + 1] (n + 1: none)."""
    lo, hi = 0, n + 1
    while lo < hi:
        mid = (lo + hi) // 2
        if stag_ref.nfa_valid(n, mid, w, h):
            hi = mid
        else:
            lo = mid + 1
    return lo


def main():
    assert stag_ref.available(), "oracle/_ref/libstag_ref.so is not built"
    L = _lib.load()
    out = {}
    for w, h in SIZES:
        kmin = np.zeros(4 * (w + h) + 64, np.int32)
        n, ls, mll = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        locs = np.zeros((72, 3))
        assert L.fid_stag_host_tables(w, h, kmin.ctypes.data, len(kmin), C.byref(n), C.byref(ls), locs.ctypes.data, C.byref(mll)) == 0
        lut, rmll, rlocs = stag_ref.host_tables(w, h)
        key = f"{w}x{h}"
        out[key + "_lut"], out[key + "_mll"], out[key + "_locs"] = lut, np.int32(rmll), rlocs
        out[key + "_kmin"] = np.array([least_k(nn, w, h) for nn in range(len(lut), n.value)], np.int32)
        print(key, len(lut), rmll, len(out[key + "_kmin"]))
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    main()
