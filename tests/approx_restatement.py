"""A NumPy restatement of k_approx's approxPolyDP (fid_kernels.hip) in the kernel's order of work -- three farthest-point passes,
the slice stack, first maximum on ties, the two `double` tests, the clean-up pass -- with its bound on the raw polygon's vertices,
and the contours the tests feed it.  Shared by tests/test_approx_stack_bound.py and tests/test_gpu_approx_bound.py."""
import os
import re

import numpy as np

import oracle

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fiducials_amd", "csrc", "fid_kernels.hip")


def source_define(name):
    m = re.search(r"^#define %s (\d+)\s*$" % name, open(SRC).read(), re.M)
    assert m, "%s is no longer a plain #define: update the tests with the kernel" % name
    return int(m.group(1))


def approx_restated(pts, rate, max_raw=None):
    """-> (rejected, raw vertex count, final vertices (k, 2), deepest stack).  max_raw: reject as soon as new_count + top exceeds it
    (the kernel's K4_MAX_RAW), checked before a pop; None: never."""
    pts = np.asarray(pts, np.int64)
    count = len(pts)
    eps = float(count) * rate
    eps *= eps
    dst, stack, deepest = [], [], 0
    rs_start = pos = 0
    le_eps = False
    for _ in range(3):
        pos = (pos + rs_start) % count
        s = pts[pos]
        if count > 1:
            idx = (pos + np.arange(1, count)) % count
            d = ((pts[idx] - s) ** 2).sum(1)
            md = int(d.max())
            if md > 0:
                rs_start = 1 + int(np.argmax(d))  # (the first index that holds the maximum)
        else:
            md = 0
        le_eps = float(md) <= eps
    if not le_eps:
        a = pos % count
        b = (rs_start + a) % count
        stack += [(b, a), (a, b)]
    else:
        dst.append(tuple(pts[pos]))
    while stack:
        deepest = max(deepest, len(stack))
        if max_raw is not None and len(dst) + len(stack) > max_raw:
            return True, None, None, deepest
        sx_, sy_ = stack.pop()
        s, e = pts[sx_], pts[sy_]
        m = (sy_ - sx_) % count - 1  # interior points
        split = None
        if m > 0:
            dx, dy = int(e[0] - s[0]), int(e[1] - s[1])
            idx = (sx_ + 1 + np.arange(m)) % count
            d = np.abs((pts[idx, 1] - s[1]) * dx - (pts[idx, 0] - s[0]) * dy)
            bt = int(np.argmax(d))
            md = float(int(d[bt]))
            if not (md * md <= eps * (float(dx) * dx + float(dy) * dy)):
                split = (sx_ + 1 + bt) % count
        if split is None:
            dst.append((int(s[0]), int(s[1])))
        else:
            stack += [(split, sy_), (sx_, split)]
            deepest = max(deepest, len(stack))
    raw = len(dst)
    # last stage: remove extra points on the [almost] straight lines
    new_count = cnt = raw
    if cnt >= 1:
        state = {"pos": cnt - 1}

        def rd():
            v = dst[state["pos"]]
            state["pos"] = (state["pos"] + 1) % cnt
            return v

        sp = rd()
        wpos = state["pos"]
        pt = rd()
        i = 0
        while i < cnt and new_count > 2:
            ep = rd()
            dx, dy = float(ep[0] - sp[0]), float(ep[1] - sp[1])
            dist = abs(float(pt[0] - sp[0]) * dy - float(pt[1] - sp[1]) * dx)
            sip = float(pt[0] - sp[0]) * (ep[0] - pt[0]) + float(pt[1] - sp[1]) * (ep[1] - pt[1])
            if dist * dist <= 0.5 * eps * (dx * dx + dy * dy) and dx != 0 and dy != 0 and sip >= 0:
                new_count -= 1
                sp = ep
                dst[wpos] = sp
                wpos = (wpos + 1) % cnt
                pt = rd()
                i += 2
                continue
            sp = pt
            dst[wpos] = sp
            wpos = (wpos + 1) % cnt
            pt = ep
            i += 1
    return False, raw, np.array(dst[:new_count], np.int32).reshape(-1, 2), deepest


def random_closed_contours(rng, n):
    """Borders of random blobs (sums of a few discs and boxes, some with a ragged rim), as cv::findContours returns them."""
    out = []
    while len(out) < n:
        m = np.zeros((240, 320), np.uint8)
        yy, xx = np.mgrid[0:240, 0:320]
        for _ in range(int(rng.integers(1, 5))):
            cx, cy, r = int(rng.integers(60, 260)), int(rng.integers(60, 180)), int(rng.integers(8, 55))
            if rng.random() < 0.5:
                m[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
            else:
                r2 = int(rng.integers(8, 55))
                m[(np.abs(xx - cx) <= r) & (np.abs(yy - cy) <= r2)] = 255
        if rng.random() < 0.5:
            rim = (m > 0) & (rng.random(m.shape) < 0.15)
            m[rim] = 0
        cs, _ = oracle.find_contours(m)
        out += [c for c in cs if len(c) >= 12]
    return out[:n]


def gate_contours(img, p):
    """The contours of every threshold scale that pass the perimeter gate: what k_approx is given."""
    h, w = img.shape
    lo, hi = p.minMarkerPerimeterRate * max(w, h), p.maxMarkerPerimeterRate * max(w, h)
    out = []
    for win in range(p.adaptiveThreshWinSizeMin, p.adaptiveThreshWinSizeMax + 1, p.adaptiveThreshWinSizeStep):
        cs, _ = oracle.find_contours(oracle.adaptive_threshold(img, win, p.adaptiveThreshConstant))
        out += [c for c in cs if lo <= len(c) <= hi]
    return out
