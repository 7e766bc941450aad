"""Host-side mirror of the reference's STag detector interface (stag_detect/include/stag/Stag.h:41-45), on top of the
C-ABI.  Under construction: `StagDetector(libraryHD, errorCorrection)` mirrors `Stag::Stag`; what exists on the MI355X so
far is the EDPF edge-detection front end of `Stag::detectMarkers` (smoothing, Prewitt gradient map, anchors, anchor
sort); the stages behind it are next.  No CPU path in this package."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import camera as _camera
from ._lib import FidError

(TAP_SMOOTH, TAP_GRAD, TAP_DIR, TAP_ANCHORS, TAP_SORTED, TAP_EDGEIMG, TAP_SEGMENTS, TAP_SEGPIX, TAP_SMOOTH2, TAP_VGRAD, TAP_VPROB,
 TAP_VSEGMENTS, TAP_LINES, TAP_VLINES, TAP_QUADS, TAP_MARKERS, TAP_GRAY) = range(17)

MARKER_DTYPE = np.dtype([("id", "i4"), ("shift", "i4"), ("corners", "f8", (4, 2)), ("center", "f8", (2,)), ("H", "f8", (3, 3)),
                         ("lineInf", "f8", (3,)), ("projectiveDistortion", "f8"), ("code", "u8")])
POSE_DTYPE = np.dtype([("id", "i4"), ("reserved", "i4"), ("rvec", "f8", (3,)), ("tvec", "f8", (3,)), ("R", "f8", (3, 3))])
TAG_DTYPE = np.dtype([("id", "i4"), ("bundle", "i4"), ("corners", "f8", (4, 3)), ("center", "f8", (3,))])  # fid_stag_tag
POSE_COV_DTYPE = np.dtype(_lib.POSE_COV_FIELDS)  # fid_pose_cov
BUNDLE_POSE_DTYPE = np.dtype([("bundle", "i4"), ("n_tags", "i4"), ("rvec", "f8", (3,)), ("tvec", "f8", (3,)), ("R", "f8", (3, 3))])
MAX_BUNDLES, MAX_TAGS_PER_BUNDLE, FRAME_LEN = 64, 12, 64  # FID_STAG_MAX_BUNDLES, FID_STAG_MAX_TAGS_PER_BUNDLE, FID_STAG_FRAME_LEN
QUAD_DTYPE = np.dtype([("corners", "f8", (4, 2)), ("lineInf", "f8", (3,)), ("projectiveDistortion", "f8")])
LINE_DTYPE = np.dtype([("a", "f8"), ("b", "f8"), ("sx", "f8"), ("sy", "f8"), ("ex", "f8"), ("ey", "f8"), ("invert", "i4"),
                       ("segmentNo", "i4"), ("firstPixelIndex", "i4"), ("len", "i4")])


def load_library(hd: int) -> np.ndarray:
    """The codewords of marker library HD<hd> (uint64, four rotations x markers): the published STag tables, extracted by
    tools/make_stag_libraries.py into fiducials_amd/data/stag_HD<hd>.bin (raw little-endian uint64, shared with the C++ host)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", f"stag_HD{hd}.bin")
    if hd not in (11, 13, 15, 17, 19, 21, 23) or not os.path.exists(path):
        raise FidError(_lib.FID_E_INVALID_ARG, "Invalid library HD. Possible values are 11, 13, 15, 17, 19, 21, or 23")
    return np.ascontiguousarray(np.fromfile(path, dtype="<u8").astype(np.uint64))


class Layout:
    """The bundles a node is configured with (stag_ros/load_yaml_tags.h): `tags` (TAG_DTYPE, ordered by bundle), and per bundle its
    frame name and whether it is a standalone tag of the `tags:` list (a bundle of one tag)."""

    def __init__(self, tags: np.ndarray, frames: list[str], standalone: np.ndarray):
        self.tags = np.ascontiguousarray(tags, dtype=TAG_DTYPE)
        self.frames = list(frames)
        self.standalone = np.asarray(standalone, dtype=bool)

    @property
    def n_bundles(self) -> int:
        return len(self.frames)


def tag_from_three_corners(tag_id: int, bundle: int, c0, c1, c2) -> np.ndarray:
    """A tag (TAG_DTYPE, one element) from the three corners the YAML gives (load_yaml_tags.h:22-30), through the C side."""
    out = np.zeros(1, TAG_DTYPE)
    c = [np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (c0, c1, c2)]
    rc = _lib.load().fid_stag_tag_from_three_corners(int(tag_id), int(bundle), c[0].ctypes.data, c[1].ctypes.data, c[2].ctypes.data, out.ctypes.data)
    if rc != _lib.FID_OK:
        raise FidError(rc, "fid_stag_tag_from_three_corners")
    return out[0]


def board_layout(ids, corners, frame: str = "board") -> Layout:
    """One bundle of the tags `ids` with `corners` (n, 4, 3): c0..c2 are taken, c3 and the centre made as the loader makes them."""
    tags = np.array([tag_from_three_corners(int(i), 0, c[0], c[1], c[2]) for i, c in zip(ids, np.asarray(corners, float))], dtype=TAG_DTYPE)
    return Layout(tags, [frame], np.zeros(1, bool))


def load_layout(path: str) -> Layout:
    """loadTagsBundles (load_yaml_tags.h:75-105) from the YAML file `rosparam load` would read, through the C loader
    (fid_stag_layout_load_file; host code, no device).  Raises FidError with the loader's message for a malformed file."""
    L = _lib.load()
    tags = np.zeros(4096, TAG_DTYPE)
    standalone = np.zeros(1024, np.uint8)
    frames = np.zeros((1024, FRAME_LEN), np.uint8)
    nt, nb = C.c_int32(0), C.c_int32(0)
    rc = L.fid_stag_layout_load_file(str(path).encode(), tags.ctypes.data, len(tags), C.byref(nt), C.byref(nb), standalone.ctypes.data,
                                     frames.ctypes.data, len(standalone))
    if rc != _lib.FID_OK:
        raise FidError(rc, L.fid_stag_layout_last_error().decode() or L.fid_strerror(rc).decode())
    names = [bytes(frames[b]).split(b"\0", 1)[0].decode() for b in range(nb.value)]
    return Layout(tags[:nt.value].copy(), names, standalone[:nb.value].astype(bool))


def _camera_call(L, name: str, K, D, camera):
    """The entry point a pose method calls and its camera arguments: `name` with K, D (plumb-bob; K None where the entry point
    allows it: no pose step), or its twin `name`_cam with camera= (fiducials_amd.camera.Camera).  The third item keeps the
    arguments' memory alive over the call."""
    if camera is not None:
        cam = _camera.resolve(K, D, camera)
        return getattr(L, name + "_cam"), (C.byref(cam.c),), cam
    Kp = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    Dp = np.zeros(5) if D is None else np.ascontiguousarray(D, dtype=np.float64).reshape(-1)[:5].copy()
    return getattr(L, name), (None if Kp is None else Kp.ctypes.data, Dp.ctypes.data), (Kp, Dp)


class StagDetector:
    def __init__(self, libraryHD: int = 21, errorCorrection: int = 7, max_width: int = 1920, max_height: int = 1080,
                 device: int = 0):
        self._L = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._L.fid_stag_create(libraryHD, errorCorrection, max_width, max_height, device, C.byref(self._ctx))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        self.shape = None
        self._words = load_library(libraryHD)  # Decoder::Decoder(libraryHD)
        rc = self._L.fid_stag_load_library(self._ctx, self._words.ctypes.data, len(self._words))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._L.fid_stag_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def edge_frontend(self, gray: np.ndarray):
        """Runs the EDPF front end on a mono8 image; results stay on the device (read them with tap())."""
        self._run(self._L.fid_stag_edge_frontend, gray)

    def detect_edges(self, gray: np.ndarray):
        """Front end + edge routing (DoDetectEdgesByED): the EdgeMap stays on the device; edge_segments() reads it."""
        self._run(self._L.fid_stag_detect_edges, gray)

    def detect_edges_validated(self, gray: np.ndarray):
        """DetectEdgesByEDPF: detect_edges() + Helmholtz validation; edge_segments(validated=True) reads the result."""
        self._run(self._L.fid_stag_detect_edges_validated, gray)

    def detect_lines(self, gray: np.ndarray):
        """DetectLinesByEDPF up to JoinCollinearLines; lines() reads the result (structured array, LINE_DTYPE)."""
        self._run(self._L.fid_stag_detect_lines, gray)

    def detect_lines_validated(self, gray: np.ndarray):
        """DetectLinesByEDPF complete (EDInterface::runEDPFandEDLines); lines(validated=True) reads EDLines::lines."""
        self._run(self._L.fid_stag_detect_lines_validated, gray)

    def detect_quads(self, gray: np.ndarray):
        """QuadDetector::detectQuads; quads() reads the result (structured array, QUAD_DTYPE)."""
        self._run(self._L.fid_stag_detect_quads, gray)

    def detect_markers_unrefined(self, gray: np.ndarray):
        """Stag::detectMarkers without the final pose refinement; markers() reads the result (MARKER_DTYPE)."""
        self._run(self._L.fid_stag_detect_markers_unrefined, gray)

    def detect_markers(self, gray: np.ndarray) -> np.ndarray:
        """Stag::detectMarkers + getMarkerList(): the markers of a mono8 image (MARKER_DTYPE), pose-refined."""
        img = np.asarray(gray)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise FidError(_lib.FID_E_INVALID_ARG, "image must be uint8 HxW")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        h, w = img.shape
        n = C.c_int32(0)
        # the markers come back in the caller's buffer (the call's own hand-over) -- reading them through the stage tap afterwards
        # was a second, synchronous device -> host copy per frame
        if getattr(self, "_mbuf", None) is None:
            self._mbuf = np.zeros(512, MARKER_DTYPE)
        rc = self._L.fid_stag_detect_markers(self._ctx, img.ctypes.data, w, h, img.strides[0], self._mbuf.ctypes.data, len(self._mbuf), C.byref(n))
        self.shape = (h, w)
        if rc == _lib.FID_E_CAPACITY:
            m = self.markers()  # more than 512 markers: the tap holds them all; a frame refused in the routing leaves no stage readable
            if len(m) > len(self._mbuf):
                return m
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return self._mbuf[:n.value].copy()

    def detect_markers_device(self, data_ptr: int, width: int, height: int, stride: int | None = None, encoding: str = "mono8") -> np.ndarray:
        """detect_markers on a frame already resident on this context's device (e.g. a torch uint8 tensor's data_ptr(); the work that
        wrote it must be complete, torch.cuda.synchronize()).  encoding: mono8, bgr8 or rgb8; stride in bytes (default: packed rows).
        Colour goes to gray in OpenCV 4.x's 15-bit form (fid_stag_detect_markers_device); tap(TAP_GRAY) reads the gray image."""
        enc = _lib.ENC.get(encoding, -1)  # (any other encoding: the library refuses it, FID_E_UNSUPPORTED)
        bpp = _lib.ENC_BYTES_PER_PIXEL.get(encoding, 1)
        stride = stride or width * bpp
        n = C.c_int32(0)
        if getattr(self, "_mbuf", None) is None:
            self._mbuf = np.zeros(512, MARKER_DTYPE)
        rc = self._L.fid_stag_detect_markers_device(self._ctx, C.c_void_p(data_ptr), width, height, stride, enc, self._mbuf.ctypes.data,
                                                    len(self._mbuf), C.byref(n))
        if rc == _lib.FID_OK or rc == _lib.FID_E_CAPACITY:
            self.shape = (height, width)
        if rc == _lib.FID_E_CAPACITY:
            m = self.markers()
            if len(m) > len(self._mbuf):
                return m
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return self._mbuf[:n.value].copy()

    def pose_last(self, K=None, D=None, marker_size: float = 0.0, camera=None) -> np.ndarray:
        """Common::solvePnpSingle for the markers of the last detect_markers*() call (POSE_DTYPE).  K, D (plumb-bob) or camera=."""
        fn, cargs, _keep = _camera_call(self._L, "fid_stag_pose_last", K, D, camera)
        out = np.zeros(4096, POSE_DTYPE)
        n = C.c_int32(0)
        rc = fn(self._ctx, *cargs, float(marker_size), out.ctypes.data, len(out), C.byref(n))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return out[:n.value].copy()

    def set_layout(self, layout: "Layout | None"):
        """The context's bundles (fid_stag_set_layout); None or an empty layout clears it."""
        tags = np.zeros(0, TAG_DTYPE) if layout is None else np.ascontiguousarray(layout.tags, dtype=TAG_DTYPE)
        nb = 0 if layout is None or len(tags) == 0 else layout.n_bundles
        rc = self._L.fid_stag_set_layout(self._ctx, tags.ctypes.data if len(tags) else None, len(tags), nb)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        self.layout = layout if len(tags) else None

    def bundle_pose_last(self, K=None, D=None, camera=None) -> np.ndarray:
        """Common::solvePnpBundle for the markers of the last detect_markers*() call, on the device (BUNDLE_POSE_DTYPE): one record per
        bundle of which a tag was found, in bundle order.  K, D (plumb-bob) or camera=."""
        fn, cargs, _keep = _camera_call(self._L, "fid_stag_bundle_pose_last", K, D, camera)
        out = np.zeros(MAX_BUNDLES, BUNDLE_POSE_DTYPE)
        n = C.c_int32(0)
        rc = fn(self._ctx, *cargs, out.ctypes.data, len(out), C.byref(n))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return out[:n.value].copy()

    def bundle_pose(self, K=None, D=None, markers: np.ndarray = None, camera=None) -> np.ndarray:
        """The same kernel on markers handed in from the host (MARKER_DTYPE; id, corners and center are read).  K, D (plumb-bob) or
        camera=."""
        fn, cargs, _keep = _camera_call(self._L, "fid_stag_bundle_pose", K, D, camera)
        m = np.ascontiguousarray(markers, dtype=MARKER_DTYPE)
        out = np.zeros(MAX_BUNDLES, BUNDLE_POSE_DTYPE)
        n = C.c_int32(0)
        rc = fn(self._ctx, *cargs, m.ctypes.data if len(m) else None, len(m), out.ctypes.data, len(out), C.byref(n))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return out[:n.value].copy()

    # -- the covariance of the poses (fid_abi.h: "pose covariance"): the twin's records and POSE_COV_DTYPE records beside them
    @staticmethod
    def _cov_camera(K, D, camera):
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        return cam

    def pose_cov_last(self, K=None, D=None, marker_size: float = 0.0, camera=None, sigma_px: float = 1.0):
        """pose_last with the covariance of every pose (fid_stag_pose_last_cov_cam): (POSE_DTYPE, POSE_COV_DTYPE) arrays."""
        cam = self._cov_camera(K, D, camera)
        out = np.zeros(4096, POSE_DTYPE)
        cov = np.zeros(len(out), POSE_COV_DTYPE)
        n = C.c_int32(0)
        rc = self._L.fid_stag_pose_last_cov_cam(self._ctx, C.byref(cam.c), float(marker_size), out.ctypes.data, len(out), C.byref(n), float(sigma_px),
                                                cov.ctypes.data)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return out[:n.value].copy(), cov[:n.value].copy()

    def bundle_pose_cov_last(self, K=None, D=None, camera=None, sigma_px: float = 1.0):
        """bundle_pose_last with the covariance of every bundle pose (fid_stag_bundle_pose_last_cov_cam)."""
        cam = self._cov_camera(K, D, camera)
        out = np.zeros(MAX_BUNDLES, BUNDLE_POSE_DTYPE)
        cov = np.zeros(len(out), POSE_COV_DTYPE)
        n = C.c_int32(0)
        rc = self._L.fid_stag_bundle_pose_last_cov_cam(self._ctx, C.byref(cam.c), out.ctypes.data, len(out), C.byref(n), float(sigma_px), cov.ctypes.data)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return out[:n.value].copy(), cov[:n.value].copy()

    def bundle_pose_cov(self, K=None, D=None, markers: np.ndarray = None, camera=None, sigma_px: float = 1.0):
        """bundle_pose with the covariance of every bundle pose (fid_stag_bundle_pose_cov_cam)."""
        cam = self._cov_camera(K, D, camera)
        m = np.ascontiguousarray(markers, dtype=MARKER_DTYPE)
        out = np.zeros(MAX_BUNDLES, BUNDLE_POSE_DTYPE)
        cov = np.zeros(len(out), POSE_COV_DTYPE)
        n = C.c_int32(0)
        rc = self._L.fid_stag_bundle_pose_cov_cam(self._ctx, C.byref(cam.c), m.ctypes.data if len(m) else None, len(m), out.ctypes.data, len(out),
                                                  C.byref(n), float(sigma_px), cov.ctypes.data)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return out[:n.value].copy(), cov[:n.value].copy()

    def queue_stats(self) -> tuple[int, int]:
        """(frames enqueued ahead of their own counts, how many of them had to be run again on the counted road)."""
        q, r = C.c_int32(0), C.c_int32(0)
        self._L.fid_stag_queue_stats(self._ctx, C.byref(q), C.byref(r))
        return q.value, r.value

    def markers(self) -> np.ndarray:
        return self.tap(TAP_MARKERS)

    def quads(self) -> np.ndarray:
        return self.tap(TAP_QUADS)

    def lines(self, validated: bool = False) -> np.ndarray:
        return self.tap(TAP_VLINES if validated else TAP_LINES)

    def edge_segments(self, validated: bool = False):
        """List of (n_i, 2) int32 arrays of (r, c): EdgeMap::segments after detect_edges() / detect_edges_validated()."""
        segs = self.tap(TAP_VSEGMENTS if validated else TAP_SEGMENTS).reshape(-1, 2)
        pix = self.tap(TAP_SEGPIX).reshape(-1, 2)
        return [pix[a:a + n] for a, n in segs]

    def _run(self, fn, gray):
        img = np.asarray(gray)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise FidError(_lib.FID_E_INVALID_ARG, "image must be uint8 HxW")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        h, w = img.shape
        rc = fn(self._ctx, img.ctypes.data, w, h, img.strides[0])
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        self.shape = (h, w)

    def tap(self, which: int) -> np.ndarray:
        n = self._L.fid_stag_tap_bytes(self._ctx, which)
        buf = np.zeros(max(n, 0), np.uint8)
        if n:
            rc = self._L.fid_stag_tap_read(self._ctx, which, buf.ctypes.data, n)
            if rc != _lib.FID_OK:
                raise FidError(rc, self._L.fid_strerror(rc).decode())
        h, w = self.shape
        if which in (TAP_SMOOTH, TAP_DIR, TAP_ANCHORS, TAP_EDGEIMG, TAP_SMOOTH2, TAP_GRAY):
            return buf.reshape(h, w)
        if which in (TAP_GRAD, TAP_VGRAD):
            return buf.view(np.int16).reshape(h, w)
        if which == TAP_VPROB:
            return buf.view(np.float64)
        if which == TAP_MARKERS:
            return buf.view(MARKER_DTYPE)
        if which == TAP_QUADS:
            return buf.view(QUAD_DTYPE)
        if which in (TAP_LINES, TAP_VLINES):
            return buf.view(LINE_DTYPE)
        return buf.view(np.int32)


class StagPool:
    """Throughput mode (fid_stag_detect_markers_batch): `n_contexts` frame slots.  The frames are a GRID DIMENSION -- the slots
    are cut into groups (32 slots where the pool has at least 64, else two groups; FID_STAG_GROUP overrides), a group carries its
    frames through the pipeline in lockstep on one stream, every kernel launched once per group (fid_stag_batch.h: frame 0's
    arguments + 32 bytes per further frame, round 6), a host thread per group.  Nothing depends on how many hardware queues the HIP
    runtime was given.  A slot is ~0.66 GB for 1080p; 256 slots: 7.9 - 8.2 k frames/s, 32 slots: ~3.5 k.
    detect_markers_batch(frames[F, H, W]) -> (markers per frame, poses per frame)."""

    def __init__(self, libraryHD: int = 21, errorCorrection: int = 7, n_contexts: int = 32, max_width: int = 1920, max_height: int = 1080,
                 device: int = 0):
        self.dets = [StagDetector(libraryHD, errorCorrection, max_width, max_height, device) for _ in range(n_contexts)]
        self._L = self.dets[0]._L
        self._arr = (C.c_void_p * n_contexts)(*[d._ctx.value for d in self.dets])

    def close(self):
        for d in self.dets:
            d.close()

    def set_layout(self, layout: "Layout | None"):
        """The same layout on every slot (what detect_bundles_batch asks for)."""
        for d in self.dets:
            d.set_layout(layout)

    def _n_bundles(self) -> int:
        lay = getattr(self.dets[0], "layout", None)
        return lay.n_bundles if lay is not None else 0

    def detect_bundles_batch(self, frames: np.ndarray, K=None, D=None, marker_size: float = 0.18, cap_per_frame: int = 64, camera=None):
        """detect_markers_batch with the bundle step behind the marker pose (fid_stag_detect_bundles_batch)
        -> (markers per frame, poses per frame, bundle poses per frame)."""
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        F, h, w = fr.shape
        nb = max(self._n_bundles(), 1)
        markers = np.zeros((F, cap_per_frame), MARKER_DTYPE)
        poses = np.zeros((F, cap_per_frame), POSE_DTYPE)
        bposes = np.zeros((F, nb), BUNDLE_POSE_DTYPE)
        counts, bcounts = np.zeros(max(F, 1), np.int32), np.zeros(max(F, 1), np.int32)
        fn, cargs, _keep = _camera_call(self._L, "fid_stag_detect_bundles_batch", K, D, camera)
        rc = fn(self._arr, len(self.dets), fr.ctypes.data, F, w, h, w, w * h, *cargs,
                                                   float(marker_size), markers.ctypes.data, poses.ctypes.data, cap_per_frame, counts.ctypes.data,
                                                   bposes.ctypes.data, bcounts.ctypes.data)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return ([markers[f, :counts[f]] for f in range(F)], [poses[f, :counts[f]] for f in range(F)],
                [bposes[f, :bcounts[f]] for f in range(F)])

    def detect_bundles_batch_device(self, data_ptr: int, nframes: int, width: int, height: int, K=None, D=None, stride: int | None = None,
                                    frame_stride: int | None = None, encoding: str = "mono8", marker_size: float = 0.18, cap_per_frame: int = 64,
                                    camera=None):
        """detect_bundles_batch on frames already resident on the pool's device (fid_stag_detect_bundles_batch_device)."""
        enc = _lib.ENC.get(encoding, -1)
        bpp = _lib.ENC_BYTES_PER_PIXEL.get(encoding, 1)
        stride = stride or width * bpp
        frame_stride = frame_stride or stride * height
        nb = max(self._n_bundles(), 1)
        markers = np.zeros((nframes, cap_per_frame), MARKER_DTYPE)
        poses = np.zeros((nframes, cap_per_frame), POSE_DTYPE)
        bposes = np.zeros((nframes, nb), BUNDLE_POSE_DTYPE)
        counts, bcounts = np.zeros(max(nframes, 1), np.int32), np.zeros(max(nframes, 1), np.int32)
        fn, cargs, _keep = _camera_call(self._L, "fid_stag_detect_bundles_batch_device", K, D, camera)
        rc = fn(self._arr, len(self.dets), C.c_void_p(data_ptr), nframes, width, height, stride, frame_stride,
                                                          enc, *cargs, float(marker_size), markers.ctypes.data,
                                                          poses.ctypes.data, cap_per_frame, counts.ctypes.data, bposes.ctypes.data, bcounts.ctypes.data)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return ([markers[f, :counts[f]] for f in range(nframes)], [poses[f, :counts[f]] for f in range(nframes)],
                [bposes[f, :bcounts[f]] for f in range(nframes)])

    def detect_markers_batch(self, frames: np.ndarray, K=None, D=None, marker_size: float = 0.18, cap_per_frame: int = 64, camera=None):
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        F, h, w = fr.shape
        markers = np.zeros((F, cap_per_frame), MARKER_DTYPE)
        poses = np.zeros((F, cap_per_frame), POSE_DTYPE)
        counts = np.zeros(F, np.int32)
        fn, cargs, _keep = _camera_call(self._L, "fid_stag_detect_markers_batch", K, D, camera)
        rc = fn(self._arr, len(self.dets), fr.ctypes.data, F, w, h, w, w * h,
                                                   *cargs, float(marker_size),
                                                   markers.ctypes.data, poses.ctypes.data, cap_per_frame, counts.ctypes.data)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return [markers[f, :counts[f]] for f in range(F)], [poses[f, :counts[f]] for f in range(F)]

    def detect_markers_batch_device(self, data_ptr: int, nframes: int, width: int, height: int, stride: int | None = None,
                                    frame_stride: int | None = None, encoding: str = "mono8", K=None, D=None, marker_size: float = 0.18,
                                    cap_per_frame: int = 64, camera=None):
        """detect_markers_batch on frames already resident on the pool's device (fid_stag_detect_markers_batch_device): frame f at
        data_ptr + f * frame_stride (default: packed frames), mono8 / bgr8 / rgb8, no host staging.  -> (markers per frame, poses
        per frame)."""
        enc = _lib.ENC.get(encoding, -1)  # (any other encoding: the library refuses it, FID_E_UNSUPPORTED)
        bpp = _lib.ENC_BYTES_PER_PIXEL.get(encoding, 1)
        stride = stride or width * bpp
        frame_stride = frame_stride or stride * height
        markers = np.zeros((nframes, cap_per_frame), MARKER_DTYPE)
        poses = np.zeros((nframes, cap_per_frame), POSE_DTYPE)
        counts = np.zeros(max(nframes, 1), np.int32)
        fn, cargs, _keep = _camera_call(self._L, "fid_stag_detect_markers_batch_device", K, D, camera)
        rc = fn(self._arr, len(self.dets), C.c_void_p(data_ptr), nframes, width, height, stride,
                                                          frame_stride, enc, *cargs,
                                                          float(marker_size), markers.ctypes.data, poses.ctypes.data, cap_per_frame,
                                                          counts.ctypes.data)
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        return [markers[f, :counts[f]] for f in range(nframes)], [poses[f, :counts[f]] for f in range(nframes)]
