#!/usr/bin/env python3
"""JPEG encoding on the device against the route it replaces (run on the GPU box), one JSON document:
  * fid_jpeg_encode_device on batches of 1, 16 and 256 1920x1080 marker frames in HBM (BGR8, quality 80, 4:2:0): ms per call by the
    host clock (the call returns when the files are in host memory) and the device time of its launches from events on the context's
    stream (fid_jpeg_enc_last_ms), after warm-up, over at least a second of calls; frames/s; bytes that cross the link per frame;
  * the parent route for the same frames, timed in the same loop, alternating with the device route: the raw frames copied to the
    host (a plain device -> host copy, what fid_jpeg_marker_image does) and encoded by libjpeg-turbo (Pillow) on one core, per frame
    (at most 16 frames of the batch per round: the route's cost per frame does not depend on the batch), with its spread;
  * kernel by kernel, from one `rocprofv3 --kernel-trace --stats` run of its own (a child process), and the transform kernel's
    achieved bytes/s against the HBM peak -- bytes from the shapes: the frame read once, the coefficients written once.
Usage: python tools/gpu_jpeg_enc_bench.py [--out profiles/jpeg_enc_bench.json] [--no-trace] | --child BATCH CALLS"""
import csv
import glob
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()
from fiducials_amd import jpeg as fj, synth  # noqa: E402
from fiducials_amd.dictionary import get_predefined_dictionary  # noqa: E402

W, H = 1920, 1080
HBM_PEAK = 8.0e12  # bytes/s, MI355X


def frames_on_device(batch):
    d = get_predefined_dictionary("DICT_5X5_250")
    distinct = [np.stack([synth.make_frame(d, 3 + s, W, H, n_markers=20).image] * 3, -1) for s in range(min(batch, 4))]
    dev = torch.empty((batch, H, W, 3), dtype=torch.uint8, device="cuda")
    for f in range(batch):
        dev[f] = torch.from_numpy(distinct[f % len(distinct)]).cuda()
    torch.cuda.synchronize()
    return dev


def spread(ts):
    ts = np.sort(np.asarray(ts, np.float64))
    return {"median_ms": round(float(np.median(ts)), 4), "p10_ms": round(float(ts[len(ts) // 10]), 4), "p90_ms": round(float(ts[(9 * len(ts)) // 10]), 4),
            "rounds": len(ts)}


def one_batch(batch):
    from PIL import Image

    dev = frames_on_device(batch)
    enc = fj.JpegEncoder(W, H, batch)
    call = lambda: enc.encode_device(dev.data_ptr(), batch, W, H, W * 3, W * H * 3, "bgr8")  # noqa: E731
    for _ in range(3):
        files = call()
    nhost = min(batch, 16)
    wall, devms, host_copy, host_enc = [], [], [], []
    total = 0.0
    while total < 1.0 or len(wall) < 5:
        t = time.perf_counter()
        call()
        dt = time.perf_counter() - t
        total += dt
        wall.append(dt * 1e3)
        devms.append(enc.last_ms())
        if len(host_enc) < 12:  # the parent route, in turn with the device route
            t = time.perf_counter()
            raw = dev[:nhost].cpu().numpy()
            t1 = time.perf_counter()
            for f in range(nhost):
                b = io.BytesIO()
                Image.fromarray(raw[f][..., ::-1]).save(b, "JPEG", quality=80, subsampling=2)
            t2 = time.perf_counter()
            host_copy.append((t1 - t) * 1e3 / nhost)
            host_enc.append((t2 - t1) * 1e3 / nhost)
    assert b.getvalue() == files[nhost - 1]  # (the two routes make the same file)
    enc.close()
    w, h = spread(wall), spread([a + c for a, c in zip(host_copy, host_enc)])
    return {"batch": batch, "device_route_call": w, "device_route_launches": spread(devms),
            "device_route_ms_per_frame": round(w["median_ms"] / batch, 4), "device_route_frames_per_s": round(batch / w["median_ms"] * 1e3, 1),
            "bytes_over_link_per_frame": int(np.mean([len(f) for f in files])), "raw_bytes_per_frame": W * H * 3,
            "parent_route_ms_per_frame": h, "parent_route_copy_ms_per_frame": spread(host_copy), "parent_route_encode_ms_per_frame": spread(host_enc),
            "device_route_faster": bool(w["median_ms"] / batch < h["median_ms"])}


def kernel_trace(batch, calls, outdir):
    """one rocprofv3 --kernel-trace --stats run of a child that only encodes; -> {kernel: {calls, mean_us}}"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", outdir, "-o", "enc", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
           "--child", str(batch), str(calls)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    if r.returncode != 0:
        return {"error": (r.stdout + r.stderr)[-400:]}
    out = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"k_jenc_\w+(<\w+>)?", row.get("Name", ""))
                if m:
                    out[m.group(0)] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2)}
    return out


def add_kernels(doc, batch, k):
    doc[f"kernels_batch_{batch}"] = k
    dct = k.get("k_jenc_dct")
    if dct:
        nblk = (W // 8) * (H // 8 + 1) + 2 * (W // 16) * (H // 16 + 1)  # 136 and 68 rows of blocks: the MCU-padded frame
        nbytes = batch * (W * H * 3 + nblk * 128)
        doc[f"transform_kernel_batch_{batch}"] = {"bytes_from_shapes": nbytes, "bytes_per_s": round(nbytes / (dct["mean_us"] * 1e-6), 0),
                                                  "of_hbm_peak": round(nbytes / (dct["mean_us"] * 1e-6) / HBM_PEAK, 4)}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        batch, calls = int(sys.argv[2]), int(sys.argv[3])
        dev = frames_on_device(batch)
        enc = fj.JpegEncoder(W, H, batch)
        for _ in range(calls):
            enc.encode_device(dev.data_ptr(), batch, W, H, W * 3, W * H * 3, "bgr8")
        enc.close()
        return 0
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    doc = {"frame": [W, H], "quality": 80, "subsampling": "4:2:0", "batches": [one_batch(b) for b in (1, 16, 256)]}
    if "--no-trace" not in sys.argv:
        for batch, calls in ((1, 20), (256, 4)):
            with tempfile.TemporaryDirectory(prefix="jpeg_enc_trace_") as tmp:  # (the profiler's tables are read here and not kept)
                add_kernels(doc, batch, kernel_trace(batch, calls, tmp))
    text = json.dumps(doc, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
