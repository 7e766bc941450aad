#!/usr/bin/env python3
"""tests/golden/stag_ref_outputs.npz: what the reference's own STag code (oracle/_ref) returns for the images the end-to-end STag
tests of tests/test_gpu_stag.py compare against -- Stag::detectMarkers on their rendered frames, on the frames bench.py times
for cfg 5 and on three pages of the reference's PDF fixture; QuadDetector::detectQuads and DetectLinesByEDPF on their synthetic
cases -- so that those tests run where oracle/_ref cannot be built.  Keys: test_gpu_stag.ref_key (entry point, the image's
SHA-256, arguments; a tuple result as <key>#0, <key>#1, ...).  Run where oracle/_ref is built (needs /root/reference at build
time); no GPU needed."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import test_gpu_stag as t  # noqa: E402
from fiducials_amd import synth  # noqa: E402
from fiducials_amd.stag import load_library  # noqa: E402
from oracle import stag_ref  # noqa: E402


def main():
    assert stag_ref.available(), "oracle/_ref/libstag_ref.so is not built"
    out = {}

    def add(call, img, *args):
        key = t.ref_key(call, img, *args)
        got = getattr(stag_ref, call)(img, *args)
        if isinstance(got, tuple):
            out.update({f"{key}#{i}": np.asarray(v) for i, v in enumerate(got)})
        else:
            out[key] = got

    for cases, modes in ((t.UNREFINED_CASES, (False,)), (t.REFINED_CASES, (True, False))):
        for hd, ec, (w, h), n, seed in cases:
            img = synth.make_stag_frame(load_library(hd), seed, w, h, n).image
            for refine in modes:
                add("detect_markers", img, hd, ec, refine)
    for f in bench.make_stag_frames(bench.shard_seeds(0, 1, bench.STAG_UNIQUE, "stag")):
        add("detect_markers", f, bench.STAG_HD, bench.STAG_EC, True)
    z = np.load(os.path.join(ROOT, "tests", "golden", "stag_hd11_pdf.npz"))
    for page in (0, 7, 14):
        add("detect_markers", z["gray"][page], 11, 2, False)
    for case in sorted(t.QUAD_CASES):
        add("detect_quads", t.QUAD_CASES[case]())
    for case in sorted(t.VALID_CASES):
        add("detect_lines", t.VALID_CASES[case]())
    np.savez_compressed(t.REF_OUTPUTS, **out)
    print(len(out), "arrays ->", t.REF_OUTPUTS)


if __name__ == "__main__":
    main()
