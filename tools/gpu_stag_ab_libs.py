#!/usr/bin/env python3
"""Two builds of the library on the same random STag frames (three image sizes, 0-20 markers, noise, blank frames): markers, poses
and refusals must be the same bytes frame by frame -- a new kernel against the build whose results were checked against the
reference's code in the rounds before.  A second leg sends the 1280 x 720 marker frames among them through
StagPool.detect_markers_batch, the group road (frames as a grid dimension, fid_stag_batch.h): a call of 3 frames, one of them
blank, so that the frames of a group record different launch sites, and a call of 32, one full group of a 64-slot pool.
The frames are rendered once, on up to 16 host cores (a 1080p frame takes ~1 s of one), and handed to both builds as files; each
build runs in a child process of its own under a time limit (AB_CHILD_TIMEOUT seconds, default 600).
Usage: gpu_stag_ab_libs.py <libA.so> <libB.so> [n_frames] [seed]"""
import hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fiducials_amd import stag as fstag, synth


def render(job):
    i, seed, path = job
    rng = np.random.default_rng([seed, i])
    w, h = ((1920, 1080), (1280, 720), (960, 540))[int(rng.integers(0, 3))]
    kind = rng.random()
    if kind < 0.05:
        img = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
    elif kind < 0.12:
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    else:
        img = synth.make_stag_frame(render.words, 12000 + 7 * seed + i, w, h, int(rng.integers(1, 21))).image
        if rng.random() < 0.3:
            img = np.clip(img.astype(np.int32) + rng.integers(-10, 11, img.shape), 0, 255).astype(np.uint8)
    np.save(path, img)
    return kind >= 0.12 and (w, h) == (1280, 720)


if os.environ.get("AB_CHILD") == "1":
    from fiducials_amd._lib import FidError
    n, td = int(sys.argv[1]), sys.argv[2]
    hd = [int(x) for x in sys.argv[3].split(",") if x][:32]  # the first 1280 x 720 frames with markers, for the group leg
    load = lambda i: np.load(os.path.join(td, f"{i}.npy"))
    det = fstag.StagDetector(21, 7, max_width=1920, max_height=1080)
    K = np.array([[1400.0, 0, 960.0], [0, 1400.0, 540.0], [0, 0, 1]])
    out = []
    for i in range(n):
        try:
            m = det.detect_markers(load(i))
            p = det.pose_last(K, None, 0.18)
            segs = det.edge_segments(validated=True)
            hs = hashlib.sha256(m.tobytes() + p.tobytes() + b"".join(s.tobytes() for s in segs) + det.lines(validated=True).tobytes()).hexdigest()[:16]
            out.append([hs, int(len(m))])
        except FidError as e:
            out.append(["refused %d" % e.status, 0])
    det.close()
    if hd:
        pool = fstag.StagPool(21, 7, n_contexts=64, max_width=1280, max_height=720)
        full = np.stack([load(hd[k % len(hd)]) for k in range(32)])
        for frames in (np.stack([full[0], np.full((720, 1280), 128, np.uint8), full[len(hd) - 1]]), full):
            try:
                ms, ps = pool.detect_markers_batch(frames, K, None, 0.18)
                out += [[hashlib.sha256(m.tobytes() + p.tobytes()).hexdigest()[:16], int(len(m))] for m, p in zip(ms, ps)]
            except FidError as e:
                out.append(["group of %d refused %d" % (len(frames), e.status), 0])
        pool.close()
    print(json.dumps(out))
    sys.exit(0)
a, b = sys.argv[1], sys.argv[2]
n = int(sys.argv[3]) if len(sys.argv) > 3 else 60
seed = int(sys.argv[4]) if len(sys.argv) > 4 else 1
res = []
with tempfile.TemporaryDirectory() as td:
    import multiprocessing as mp
    render.words = fstag.load_library(21)
    with mp.get_context("fork").Pool(min(16, os.cpu_count() or 1)) as workers:  # (this process never opens the GPU)
        is_hd = workers.map(render, [(i, seed, os.path.join(td, f"{i}.npy")) for i in range(n)], chunksize=1)
    hd = ",".join(str(i) for i in range(n) if is_hd[i])
    for lib in (a, b):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), td, hd], env=dict(os.environ, AB_CHILD="1", FID_LIB=lib), capture_output=True,
                               text=True, timeout=int(os.environ.get("AB_CHILD_TIMEOUT", "600")))
        except subprocess.TimeoutExpired:
            print("time limit passed with", lib)
            sys.exit(3)
        lines = [l for l in p.stdout.splitlines() if l.startswith("[")]
        if p.returncode != 0 or not lines:  # (a fault or an abort: nothing more is started)
            print("no result from", lib, "exit status", p.returncode, p.stderr[-500:])
            sys.exit(2)
        res.append(json.loads(lines[-1]))
bad = [i for i, (x, y) in enumerate(zip(*res)) if x != y] if len(res[0]) == len(res[1]) else [-1]
print(f"stag A/B of two builds: {n} frames (seed {seed}) + {len(res[0]) - n} through the group road, markers {sum(x[1] for x in res[0])}, "
      f"refused {sum(x[0].startswith('refused') for x in res[0])}, mismatches {len(bad)} {bad[:10]}")
sys.exit(1 if bad else 0)
