"""Host-side mirror of the reference's detector interface, on top of the C-ABI.

`ArucoDetector.detect_markers(image)` has the argument meaning and result shape of
`aruco::detectMarkers(image, dictionary, corners, ids, detectorParams)` as aruco_detect calls it
(aruco_detect/src/aruco_detect.cpp:350): corners are (n, 4, 2) float32 in TL,TR,BR,BL order of the
canonical marker, ids (n,) int32, in OpenCV's output order.  `estimate_pose_single_markers` mirrors
`FiducialsNode::estimatePoseSingleMarkers` (:223-255) plus the per-marker error/area values that
poseEstimateCallback publishes (:480-497).

Everything here runs on the MI355X through libfid_amd.so; there is no CPU path in this package.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import camera as _camera
from ._lib import FidCandidate, FidDict, FidError, FidLimits, FidMarker, FidParams, FidPoseOut
from .dictionary import Dictionary, get_predefined_dictionary


def default_params() -> FidParams:
    p = FidParams()
    _lib.load().fid_default_params(C.byref(p))
    return p


@dataclass
class PoseResult:
    rvecs: np.ndarray  # (n, 3)
    tvecs: np.ndarray  # (n, 3)
    image_error: np.ndarray  # (n,)
    object_error: np.ndarray
    fiducial_area: np.ndarray


_MARKER_DT = np.dtype([("id", "<i4"), ("corners", "<f4", (8,))])  # fid_marker
MAP_ENTRY_DTYPE = np.dtype([("id", "<i4"), ("reserved0", "<i4"), ("len", "<f8"), ("R", "<f8", (3, 3)), ("t", "<f8", (3,))])  # fid_map_entry
MAP_POSE_DTYPE = np.dtype([("n_markers", "<i4"), ("n_over", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("R", "<f8", (3, 3)),
                           ("cam_R", "<f8", (3, 3)), ("cam_t", "<f8", (3,)), ("image_error", "<f8")])  # fid_map_pose_out
POSE_COV_DTYPE = np.dtype(_lib.POSE_COV_FIELDS)  # fid_pose_cov
MAP_POSE_COV_DTYPE = np.dtype([("pose", POSE_COV_DTYPE), ("cov_cam_pose", "<f8", (6, 6))])  # fid_map_pose_cov
MAP_ROBUST_DTYPE = _lib.MAP_ROBUST_DTYPE  # fid_map_robust_out
CHARUCO_CORNER_DTYPE = _lib.CHARUCO_CORNER_DTYPE  # fid_charuco_corner
CHARUCO_POSE_DTYPE = _lib.CHARUCO_POSE_DTYPE  # fid_charuco_pose_out
DIAMOND_DTYPE = _lib.DIAMOND_DTYPE  # fid_diamond
RIG_POSE_DTYPE = _lib.RIG_POSE_DTYPE  # fid_rig_pose_out


def map_robust_outlier_positions(rec) -> np.ndarray:
    """The used-marker indices k (0 .. n_used - 1) whose bit is set in a MAP_ROBUST_DTYPE record's outlier_mask."""
    mask = np.asarray(rec["outlier_mask"], np.uint64).reshape(4)
    return np.array([k for k in range(int(rec["n_used"])) if (int(mask[k >> 6]) >> (k & 63)) & 1], np.int64)


def map_robust_outlier_ids(rec, ids, map_ids) -> np.ndarray:
    """The fiducial ids a MAP_ROBUST_DTYPE record leaves out, in list order: ids is the frame's id list as it was handed to the
    call, map_ids the ids the context's map names.  The used markers are recounted as the kernel counts them (list order, ids the
    map does not name skipped, an id seen twice left out altogether, the first MAP_MAX_USED kept) and the record's mask is read
    against them."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    named = set(int(i) for i in np.asarray(map_ids).reshape(-1))
    vals, counts = np.unique(ids, return_counts=True)
    twice = set(int(v) for v, c in zip(vals, counts) if c > 1)
    used = [int(i) for i in ids if int(i) in named and int(i) not in twice][:_lib.MAP_MAX_USED]
    if len(used) != int(rec["n_used"]):
        raise ValueError(f"the record counts {int(rec['n_used'])} used markers, this id list and map give {len(used)}")
    return np.array([used[k] for k in map_robust_outlier_positions(rec)], np.int64)
_POSE_DT = np.dtype([("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("image_error", "<f8"), ("object_error", "<f8"), ("fiducial_area", "<f8")])


def _poses_view_to_result(v) -> PoseResult:
    """v: a structured view (_POSE_DT) of n fid_pose_out records; copies (the buffer is reused by the next call)."""
    return PoseResult(rvecs=v["rvec"].copy(), tvecs=v["tvec"].copy(), image_error=v["image_error"].copy(),
                      object_error=v["object_error"].copy(), fiducial_area=v["fiducial_area"].copy())


def _poses_to_result(arr, n) -> PoseResult:
    return PoseResult(
        rvecs=np.array([list(arr[i].rvec) for i in range(n)], dtype=np.float64).reshape(n, 3),
        tvecs=np.array([list(arr[i].tvec) for i in range(n)], dtype=np.float64).reshape(n, 3),
        image_error=np.array([arr[i].image_error for i in range(n)]),
        object_error=np.array([arr[i].object_error for i in range(n)]),
        fiducial_area=np.array([arr[i].fiducial_area for i in range(n)]),
    )


def map_entry_from_rpy(fid: int, length: float, xyz, rpy_deg) -> np.ndarray:
    """One map entry (MAP_ENTRY_DTYPE scalar) from a position and roll, pitch, yaw in degrees, the map file's convention
    (fid_map_entry_from_rpy)."""
    L = _lib.load()
    e = np.zeros(1, MAP_ENTRY_DTYPE)
    p = np.ascontiguousarray(xyz, dtype=np.float64).reshape(3)
    a = np.ascontiguousarray(rpy_deg, dtype=np.float64).reshape(3)
    rc = L.fid_map_entry_from_rpy(int(fid), float(length), p.ctypes.data, a.ctypes.data, e.ctypes.data)
    if rc != _lib.FID_OK:
        raise FidError(rc, (L.fid_map_last_error() or b"").decode() or L.fid_strerror(rc).decode())
    return e[0]


def map_entries(ids, lengths, Rs, ts) -> np.ndarray:
    """Map entries from transforms T_map_fid given as matrices: ids (n,), lengths scalar or (n,), Rs (n, 3, 3), ts (n, 3)."""
    ids = np.asarray(ids, np.int32).reshape(-1)
    e = np.zeros(len(ids), MAP_ENTRY_DTYPE)
    e["id"] = ids
    e["len"] = lengths
    e["R"] = np.asarray(Rs, np.float64).reshape(len(ids), 3, 3)
    e["t"] = np.asarray(ts, np.float64).reshape(len(ids), 3)
    return e


def save_map(path: str, markers) -> None:
    """The file fiducial_slam reads as its map_file (fid_map_save_file): the FIXED and SOLVED records of build_map's markers."""
    L = _lib.load()
    m = np.ascontiguousarray(markers, dtype=_lib.BUILD_MARKER_DTYPE).reshape(-1)
    rc = L.fid_map_save_file(str(path).encode(), m.ctypes.data if len(m) else None, len(m))
    if rc != 0:
        raise FidError(rc, L.fid_map_last_error().decode())


def load_map(path: str, fiducial_len: float, fiducial_len_override: dict | None = None):
    """A fiducial_slam map file (fiducial_slam/src/map.cpp:541-625; fid_map_load_file): returns (entries, n_skipped) -- the
    entries as MAP_ENTRY_DTYPE with len = fiducial_len, or its per-id override (the node's fiducial_len_override list), and the
    number of lines that were passed over."""
    L = _lib.load()
    n, skipped = C.c_int32(0), C.c_int32(0)
    e = np.zeros(_lib.MAP_MAX_ENTRIES, MAP_ENTRY_DTYPE)
    rc = L.fid_map_load_file(str(path).encode(), float(fiducial_len), e.ctypes.data, len(e), C.byref(n), C.byref(skipped))
    if rc != _lib.FID_OK:
        raise FidError(rc, (L.fid_map_last_error() or b"").decode() or L.fid_strerror(rc).decode())
    e = e[:n.value].copy()
    for k, v in (fiducial_len_override or {}).items():
        e["len"][e["id"] == int(k)] = float(v)
    return e, int(skipped.value)


class ArucoDetector:
    def __init__(self, dictionary: Dictionary | int | str = 7, params: FidParams | None = None, device: int = 0,
                 max_width: int = 1920, max_height: int = 1080, max_batch: int = 1, max_markers: int = 256,
                 max_candidates: int = 2048, max_starts: int = 0, max_contours: int = 0, max_points: int = 0):
        self._L = _lib.load()
        self.dictionary = dictionary if isinstance(dictionary, Dictionary) else get_predefined_dictionary(dictionary)
        self.params = params or default_params()
        d = self.dictionary
        self._dict_bytes = np.ascontiguousarray(d.bytes_list, dtype=np.uint8)
        fd = FidDict(d.marker_size, d.max_correction_bits, d.n_markers, 0, self._dict_bytes.ctypes.data)
        lim = FidLimits()  # zero = "library default for this context size" (fid_create)
        lim.max_width, lim.max_height, lim.max_batch = max_width, max_height, max_batch
        lim.max_markers_per_frame, lim.max_candidates_per_frame = max_markers, max_candidates
        if max_starts:
            lim.max_starts_per_frame = max_starts
        if max_contours:
            lim.max_contours_per_frame = max_contours
        if max_points:
            lim.max_points_per_frame = max_points
        self.limits = lim
        self._ctx = C.c_void_p()
        rc = self._L.fid_create(C.byref(self.params), C.byref(fd), C.byref(lim), device, C.byref(self._ctx))
        if rc != _lib.FID_OK:
            raise FidError(rc, self._L.fid_strerror(rc).decode())
        self.device = device
        self.max_markers = max_markers
        self.max_batch = max_batch
        self._out = (FidMarker * (max_batch * max_markers))()
        self._n = (C.c_int32 * max_batch)()
        self._poses = (FidPoseOut * (max_batch * max_markers))()
        # numpy views of the two result buffers: unpacking twenty markers field by field through ctypes cost the single-frame call
        # ~50 us of Python (round 5; the C-ABI call itself is unchanged)
        assert C.sizeof(FidMarker) == _MARKER_DT.itemsize and C.sizeof(FidPoseOut) == _POSE_DT.itemsize
        self._out_np = np.frombuffer(self._out, dtype=_MARKER_DT)
        self._poses_np = np.frombuffer(self._poses, dtype=_POSE_DT)
        self._last_frames = 0
        self._rig_cameras = 0  # cameras of the rig set_rig handed over (0: none)

    # -- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._L.fid_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == _lib.FID_E_CV_EXCEPTION:
            raise _lib.CvException(rc, (self._L.fid_last_error(self._ctx) or b"").decode())
        if rc != _lib.FID_OK:
            raise FidError(rc, (self._L.fid_last_error(self._ctx) or b"").decode() or self._L.fid_strerror(rc).decode())

    def set_params(self, params: FidParams):
        """dynamic_reconfigure path (aruco_detect.cpp:257-298)."""
        self._check(self._L.fid_set_params(self._ctx, C.byref(params)))
        self.params = params

    # -- detection ----------------------------------------------------------------------------
    def _unpack(self, nframes):
        res = []
        mm = self.max_markers
        for f in range(nframes):
            n = max(int(self._n[f]), 0)  # (-1: the frame on which the reference's detectMarkers throws)
            v = self._out_np[f * mm:f * mm + n]
            res.append((v["corners"].reshape(n, 4, 2).copy(), v["id"].copy()))
        self._last_frames = nframes
        return res

    def detect_markers(self, image: np.ndarray, encoding: str | None = None):
        """One frame from host memory.  image: (H, W) uint8 mono8, (H, W, 3) bgr8/rgb8 or (H, W, 4) bgra8/rgba8 (default bgr8, the
        encoding imageCallback requests from cv_bridge, :348).  Returns (corners, ids)."""
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim not in (2, 3):
            raise FidError(_lib.FID_E_INVALID_ARG, "image must be uint8 HxW or HxWx3")
        if encoding is None:
            encoding = "mono8" if img.ndim == 2 else ("bgra8" if img.shape[2] == 4 else "bgr8")
        if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != img.shape[2]):
            img = np.ascontiguousarray(img)
        h, w = img.shape[:2]
        rc = self._L.fid_detect(self._ctx, img.ctypes.data, w, h, img.strides[0], _lib.ENC[encoding], self._out,
                                self.max_markers, self._n)
        self._check(rc)
        return self._unpack(1)[0]

    def detect_image(self, data, width: int, height: int, step: int, encoding: str, is_bigendian: bool = False):
        """One sensor_msgs/Image by its fields (data = the message bytes), in ANY encoding cv_bridge::toCvCopy(msg, BGR8) converts
        (aruco_detect.cpp:348): the five 8-bit layouts, and since ABI 7 bayer_{rggb,bggr,gbrg,grbg}8, mono16 / bgr16 / rgb16 / bgra16 /
        rgba16 (either byte order) and yuv422 -- the conversion is the device's first kernel, the message bytes are what crosses
        PCIe.  Returns (corners, ids)."""
        buf = np.ascontiguousarray(data).view(np.uint8).reshape(-1) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        if encoding not in _lib.ENC:
            raise FidError(_lib.FID_E_UNSUPPORTED, f"cv_bridge exception: unsupported encoding {encoding}")
        width, height, step = int(width), int(height), int(step)
        if width < 1 or height < 1 or step < width * _lib.ENC_BYTES_PER_PIXEL[encoding] or buf.size < step * height:
            raise FidError(_lib.FID_E_INVALID_ARG, f"image is wrongly formed: {buf.size} bytes for step {step} x height {height} ({encoding})")
        rc = self._L.fid_detect(self._ctx, buf.ctypes.data, width, height, step, _lib.encoding_value(encoding, is_bigendian), self._out,
                                self.max_markers, self._n)
        self._check(rc)
        return self._unpack(1)[0]

    def detect_markers_batch(self, images: np.ndarray, encoding: str | None = None, unpack: bool = True, width: int | None = None):
        """Frames in host memory (pinned or pageable): they go up sub-batch by sub-batch while the call runs.  images: (F, H, W)
        mono8 / Bayer, (F, H, W, C) 8-bit colour, or -- with `width` given -- (F, H, step) message rows of a multi-byte encoding."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        if encoding is None:
            encoding = "mono8" if imgs.ndim == 3 else "bgr8"
        f, h, w = imgs.shape[:3]
        if width is not None:
            w = int(width)
        rc = self._L.fid_detect_batch(self._ctx, imgs.ctypes.data, f, w, h, imgs.strides[1], imgs.strides[0],
                                      _lib.ENC[encoding], self._out, self.max_markers, self._n)
        self._check(rc)
        self._last_frames = f
        if not unpack:
            return [int(self._n[k]) for k in range(f)]
        return self._unpack(f)

    def detect_markers_device(self, data_ptr: int, nframes: int, width: int, height: int, stride: int | None = None,
                              frame_stride: int | None = None, encoding: str = "mono8", unpack: bool = True):
        """Frames already resident in HBM (e.g. a torch uint8 tensor's data_ptr() on this device)."""
        bpp = _lib.ENC_BYTES_PER_PIXEL[encoding]
        stride = stride or width * bpp
        frame_stride = frame_stride or stride * height
        rc = self._L.fid_detect_device(self._ctx, C.c_void_p(data_ptr), nframes, width, height, stride, frame_stride,
                                       _lib.ENC[encoding], self._out, self.max_markers, self._n)
        self._check(rc)
        self._last_frames = nframes
        if not unpack:
            return [int(self._n[f]) for f in range(nframes)]
        return self._unpack(nframes)

    def submit_device(self, data_ptr: int, nframes: int, width: int, height: int, stride: int | None = None,
                      frame_stride: int | None = None, encoding: str = "mono8", after: "ArucoDetector | None" = None) -> None:
        """First half of detect_markers_device: enqueue the batch and return at once (fid_submit_device).  The frames must stay
        where they are until collect().  after = another detector: start when its batch in flight is past its chip-filling
        kernels (fid_order_after)."""
        if after is not None:
            self._check(self._L.fid_order_after(self._ctx, after._ctx))
        bpp = _lib.ENC_BYTES_PER_PIXEL[encoding]
        stride = stride or width * bpp
        frame_stride = frame_stride or stride * height
        self._check(self._L.fid_submit_device(self._ctx, C.c_void_p(data_ptr), nframes, width, height, stride, frame_stride,
                                              _lib.ENC[encoding]))
        self._submitted = nframes

    def submit_batch(self, images: np.ndarray, encoding: str | None = None, after: "ArucoDetector | None" = None) -> None:
        """First half of detect_markers_batch (fid_submit_batch): frames in host memory -- a C-contiguous uint8 array that the
        caller keeps alive and unchanged until collect()."""
        imgs = images
        if imgs.dtype != np.uint8 or not imgs.flags.c_contiguous:
            raise ValueError("submit_batch takes a C-contiguous uint8 array (no hidden copy: the memory is read until collect())")
        if encoding is None:
            encoding = "mono8" if imgs.ndim == 3 else "bgr8"
        if after is not None:
            self._check(self._L.fid_order_after(self._ctx, after._ctx))
        f, h, w = imgs.shape[:3]
        self._check(self._L.fid_submit_batch(self._ctx, imgs.ctypes.data, f, w, h, imgs.strides[1], imgs.strides[0], _lib.ENC[encoding]))
        self._submitted = f
        self._held = imgs  # (keeps the array alive)

    def collect(self, unpack: bool = True):
        """Second half: wait for the submitted batch and return what detect_markers_device would have (fid_collect)."""
        self._check(self._L.fid_collect(self._ctx, self._out, self.max_markers, self._n))
        self._held = None
        nframes = self._last_frames = self._submitted
        if not unpack:
            return [int(self._n[f]) for f in range(nframes)]
        return self._unpack(nframes)

    # -- pose ---------------------------------------------------------------------------------
    def estimate_pose_single_markers(self, corners: np.ndarray, ids: np.ndarray, fiducial_len: float, K=None, D=None,
                                     fiducial_len_override: dict | None = None, camera=None) -> PoseResult:
        """fid_pose for markers handed in from the host: K, D (plumb-bob), or camera= (fiducials_amd.camera.Camera: fid_pose_cam)."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
        n = corners.shape[0]
        mk = (FidMarker * max(n, 1))()
        lens = (C.c_double * max(n, 1))()
        for i in range(n):
            mk[i].id = int(ids[i])
            for j in range(8):
                mk[i].corners[j] = float(corners[i, j])
            lens[i] = float((fiducial_len_override or {}).get(int(ids[i]), fiducial_len))  # :241-244
        out = (FidPoseOut * max(n, 1))()
        if camera is not None:
            self._check(self._L.fid_pose_cam(self._ctx, C.byref(cam.c), mk, lens, n, float(fiducial_len), out))
            return _poses_to_result(out, n)
        Kc = (C.c_double * 9)(*np.asarray(K, dtype=np.float64).reshape(9))
        Dc = (C.c_double * 5)(*np.asarray(D, dtype=np.float64).reshape(-1)[:5])
        self._check(self._L.fid_pose(self._ctx, Kc, Dc, mk, lens, n, float(fiducial_len), out))
        return _poses_to_result(out, n)

    def estimate_pose_single_markers_cov(self, corners: np.ndarray, ids: np.ndarray, fiducial_len: float, K=None, D=None,
                                         fiducial_len_override: dict | None = None, camera=None, sigma_px: float = 1.0):
        """estimate_pose_single_markers with the covariance of every pose (fid_pose_cov_cam): (PoseResult, POSE_COV_DTYPE records).
        sigma_px: the corner noise in pixels; 0 takes the a-posteriori estimate from the residuals."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
        n = corners.shape[0]
        mk = (FidMarker * max(n, 1))()
        lens = (C.c_double * max(n, 1))()
        for i in range(n):
            mk[i].id = int(ids[i])
            for j in range(8):
                mk[i].corners[j] = float(corners[i, j])
            lens[i] = float((fiducial_len_override or {}).get(int(ids[i]), fiducial_len))
        out = (FidPoseOut * max(n, 1))()
        cov = np.zeros(max(n, 1), POSE_COV_DTYPE)
        self._check(self._L.fid_pose_cov_cam(self._ctx, C.byref(cam.c), mk, lens, n, float(fiducial_len), out, float(sigma_px), cov.ctypes.data))
        return _poses_to_result(out, n), cov[:n]

    def pose_cov_last(self, fiducial_len: float, K=None, D=None, camera=None, sigma_px: float = 1.0):
        """pose_last with the covariance of every pose (fid_pose_last_cov_cam): (list of PoseResult, list of POSE_COV_DTYPE arrays), one
        of each per frame.  The camera and sigma_px are remembered: the next detect_* call computes both in its own stream."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        cov = np.zeros(max(self._last_frames, 1) * self.max_markers, POSE_COV_DTYPE)
        self._check(self._L.fid_pose_last_cov_cam(self._ctx, C.byref(cam.c), float(fiducial_len), self._poses, self.max_markers, float(sigma_px),
                                                  cov.ctypes.data))
        res, covs = [], []
        for f in range(self._last_frames):
            n = max(int(self._n[f]), 0)
            res.append(_poses_view_to_result(self._poses_np[f * self.max_markers:f * self.max_markers + n]))
            covs.append(cov[f * self.max_markers:f * self.max_markers + n])
        return res, covs

    def project_points(self, camera, rvec, tvec, obj, jacobian: bool = False):
        """cv::projectPoints under `camera` (fid_project_points_cam: the pose kernels' own projection run as a small kernel): obj
        (n, 3) -> uv (n, 2); with jacobian=True also d(u, v) / d(rvec, tvec) as (n, 2, 6)."""
        cam = _camera.resolve(None, None, camera)
        if cam is None:
            raise ValueError("project_points needs a camera")
        o = np.ascontiguousarray(obj, dtype=np.float64).reshape(-1, 3)
        r = np.ascontiguousarray(rvec, dtype=np.float64).reshape(3)
        t = np.ascontiguousarray(tvec, dtype=np.float64).reshape(3)
        uv = np.zeros((len(o), 2))
        jac = np.zeros((len(o), 2, 6)) if jacobian else None
        self._check(self._L.fid_project_points_cam(self._ctx, C.byref(cam.c), r.ctypes.data, t.ctypes.data, o.ctypes.data if len(o) else None, len(o),
                                                   uv.ctypes.data if len(o) else None, jac.ctypes.data if jacobian and len(o) else None))
        return (uv, jac) if jacobian else uv

    def refine_contour_corners(self, contours, corners) -> np.ndarray:
        """aruco.cpp _refineCandidateLines (CORNER_REFINE_CONTOUR) for markers given by their contours (list of (n_i, 2) int
        arrays in findContours order) and quads ((m, 4, 2), corners on the contours): the device code the pipeline runs after
        `_filterDetectedMarkers` when cornerRefinementMethod = 2.  Raises CvException where the reference throws."""
        cs = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1, 2) for c in contours]
        off = np.zeros(len(cs) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(c) for c in cs])
        pts = np.ascontiguousarray(np.concatenate(cs) if cs else np.zeros((0, 2), np.int32))
        q = np.ascontiguousarray(corners, dtype=np.float32).reshape(len(cs), 8).copy()
        st = np.zeros(max(len(cs), 1), dtype=np.int32)
        self.last_refine_status = st
        self._check(self._L.fid_refine_contour_corners(self._ctx, pts.ctypes.data, off.ctypes.data, len(cs), q.ctypes.data, st.ctypes.data))
        return q.reshape(-1, 4, 2)

    def pose_last(self, fiducial_len: float, K=None, D=None, unpack: bool = True, camera=None):
        """Poses of the markers found by the last detect_* call, computed without the corners leaving HBM.  K, D (plumb-bob) or
        camera= (fid_pose_last_cam)."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        if camera is not None:
            self._check(self._L.fid_pose_last_cam(self._ctx, C.byref(cam.c), float(fiducial_len), self._poses, self.max_markers))
        else:
            Kc = (C.c_double * 9)(*np.asarray(K, dtype=np.float64).reshape(9))
            Dc = (C.c_double * 5)(*np.asarray(D, dtype=np.float64).reshape(-1)[:5])
            self._check(self._L.fid_pose_last(self._ctx, Kc, Dc, float(fiducial_len), self._poses, self.max_markers))
        if not unpack:
            return None
        res = []
        for f in range(self._last_frames):
            n = max(int(self._n[f]), 0)
            res.append(_poses_view_to_result(self._poses_np[f * self.max_markers:f * self.max_markers + n]))
        return res

    # -- the camera among the fiducials of a map ----------------------------------------------------
    def set_map(self, entries) -> None:
        """The map the camera is posed against (fid_set_map): MAP_ENTRY_DTYPE records (load_map, map_entries, map_entry_from_rpy);
        None or an empty array clears it."""
        e = np.zeros(0, MAP_ENTRY_DTYPE) if entries is None else np.ascontiguousarray(entries, dtype=MAP_ENTRY_DTYPE).reshape(-1)
        self._check(self._L.fid_set_map(self._ctx, e.ctypes.data if len(e) else None, len(e)))

    @staticmethod
    def _cam(K, D):
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        Dc = None if D is None else np.ascontiguousarray(np.asarray(D, dtype=np.float64).reshape(-1)[:5])
        return Kc, Dc

    def map_pose_last(self, K=None, D=None, camera=None) -> np.ndarray:
        """One camera pose per frame of the last detect_* / collect call (fid_map_pose_last): MAP_POSE_DTYPE records.  K, D
        (plumb-bob) or camera= (fid_map_pose_last_cam)."""
        out = np.zeros(max(self._last_frames, 1), MAP_POSE_DTYPE)
        if camera is not None:
            cam = _camera.resolve(K, D, camera)
            self._check(self._L.fid_map_pose_last_cam(self._ctx, C.byref(cam.c), out.ctypes.data, len(out)))
            return out[:self._last_frames]
        Kc, Dc = self._cam(K, D)
        self._check(self._L.fid_map_pose_last(self._ctx, Kc.ctypes.data, Dc.ctypes.data if Dc is not None else None, out.ctypes.data, len(out)))
        return out[:self._last_frames]

    def map_pose(self, K=None, D=None, corners=None, ids=None, camera=None) -> np.ndarray:
        """The same kernel on the markers of one frame handed in from the host (fid_map_pose): corners (n, 4, 2), ids (n,) in list
        order.  Returns one MAP_POSE_DTYPE record.  K, D (plumb-bob) or camera= (fid_map_pose_cam)."""
        ids = np.asarray(ids, np.int32).reshape(-1)
        mk = np.zeros(len(ids), _MARKER_DT)
        mk["id"] = ids
        mk["corners"] = np.asarray(corners, np.float32).reshape(len(ids), 8)
        out = np.zeros(1, MAP_POSE_DTYPE)
        if camera is not None:
            cam = _camera.resolve(K, D, camera)
            self._check(self._L.fid_map_pose_cam(self._ctx, C.byref(cam.c), mk.ctypes.data if len(mk) else None, len(mk), out.ctypes.data))
            return out[0]
        Kc, Dc = self._cam(K, D)
        self._check(self._L.fid_map_pose(self._ctx, Kc.ctypes.data, Dc.ctypes.data if Dc is not None else None,
                                         mk.ctypes.data if len(mk) else None, len(mk), out.ctypes.data))
        return out[0]

    def map_pose_cov_last(self, K=None, D=None, camera=None, sigma_px: float = 1.0):
        """map_pose_last with its covariance (fid_map_pose_last_cov_cam): (MAP_POSE_DTYPE records, MAP_POSE_COV_DTYPE records), one
        of each per frame; cov["cov_cam_pose"] is the camera's covariance in the map frame."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        out = np.zeros(max(self._last_frames, 1), MAP_POSE_DTYPE)
        cov = np.zeros(len(out), MAP_POSE_COV_DTYPE)
        self._check(self._L.fid_map_pose_last_cov_cam(self._ctx, C.byref(cam.c), out.ctypes.data, len(out), float(sigma_px), cov.ctypes.data))
        return out[:self._last_frames], cov[:self._last_frames]

    def map_pose_cov(self, K=None, D=None, corners=None, ids=None, camera=None, sigma_px: float = 1.0):
        """map_pose with its covariance (fid_map_pose_cov_cam): one MAP_POSE_DTYPE record and one MAP_POSE_COV_DTYPE record."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        ids = np.asarray(ids, np.int32).reshape(-1)
        mk = np.zeros(len(ids), _MARKER_DT)
        mk["id"] = ids
        mk["corners"] = np.asarray(corners, np.float32).reshape(len(ids), 8)
        out = np.zeros(1, MAP_POSE_DTYPE)
        cov = np.zeros(1, MAP_POSE_COV_DTYPE)
        self._check(self._L.fid_map_pose_cov_cam(self._ctx, C.byref(cam.c), mk.ctypes.data if len(mk) else None, len(mk), out.ctypes.data,
                                                 float(sigma_px), cov.ctypes.data))
        return out[0], cov[0]

    # -- the body that carries several cameras, among the fiducials of a map -------------------------
    def set_rig(self, cameras) -> None:
        """The rig (fid_set_rig): a sequence of camera.RigCamera, camera c of the rig taking frames c, c + C, c + 2 C, ... of a detect
        call; None or an empty sequence clears it."""
        cams = [] if cameras is None else list(cameras)
        for rc in cams:
            if not isinstance(rc, _camera.RigCamera):
                raise TypeError("set_rig takes fiducials_amd.camera.RigCamera objects")
        tab = (_lib.FidRigCamera * max(len(cams), 1))()
        for i, rc in enumerate(cams):
            C.memmove(C.byref(tab[i]), C.byref(rc.c), C.sizeof(_lib.FidRigCamera))
        self._check(self._L.fid_set_rig(self._ctx, C.cast(tab, C.c_void_p) if cams else None, len(cams)))
        self._rig_cameras = len(cams)

    def rig_pose_last(self, sigma_px: float | None = None):
        """One rig pose per time step of the last detect_* / collect call (fid_rig_pose_last): RIG_POSE_DTYPE records, frame f being
        camera f % C of step f // C.  With sigma_px (0: the a-posteriori estimate) also MAP_POSE_COV_DTYPE records, cov_cam_pose being
        the rig's covariance in the map frame: (records, covariances)."""
        steps = max(self._last_frames // max(self._rig_cameras, 1), 1)
        out = np.zeros(steps, RIG_POSE_DTYPE)
        if sigma_px is None:
            self._check(self._L.fid_rig_pose_last(self._ctx, out.ctypes.data, len(out), 0.0, None))
            return out
        cov = np.zeros(steps, MAP_POSE_COV_DTYPE)
        self._check(self._L.fid_rig_pose_last(self._ctx, out.ctypes.data, len(out), float(sigma_px), cov.ctypes.data))
        return out, cov

    def rig_pose(self, corners_per_camera, ids_per_camera, sigma_px: float | None = None):
        """The same kernel on one time step handed in from the host (fid_rig_pose): per camera of the rig, in its order, corners
        (n_c, 4, 2) and ids (n_c,) in list order.  One RIG_POSE_DTYPE record; with sigma_px (record, MAP_POSE_COV_DTYPE record)."""
        ids = [np.asarray(i, np.int32).reshape(-1) for i in ids_per_camera]
        if len(ids) != len(corners_per_camera) or len(ids) != self._rig_cameras:
            raise ValueError(f"rig_pose takes one marker list per camera of the rig ({self._rig_cameras})")
        n = np.array([len(i) for i in ids], np.int32)
        mk = np.zeros(int(n.sum()), _MARKER_DT)
        if len(mk):
            mk["id"] = np.concatenate(ids)
            mk["corners"] = np.concatenate([np.asarray(c, np.float32).reshape(len(i), 8) for c, i in zip(corners_per_camera, ids)])
        out = np.zeros(1, RIG_POSE_DTYPE)
        cov = None if sigma_px is None else np.zeros(1, MAP_POSE_COV_DTYPE)
        self._check(self._L.fid_rig_pose(self._ctx, mk.ctypes.data if len(mk) else None, n.ctypes.data, out.ctypes.data,
                                         0.0 if sigma_px is None else float(sigma_px), None if cov is None else cov.ctypes.data))
        return out[0] if cov is None else (out[0], cov[0])

    @staticmethod
    def _robust_opts(inlier_px, min_markers):
        if inlier_px is None:
            raise ValueError("map_pose_robust needs inlier_px (recommended: _lib.MAP_ROBUST_INLIER_PX); the ABI has no default")
        return _lib.FidMapRobustOpts(float(inlier_px), int(min_markers), 0)

    def map_pose_robust(self, K=None, D=None, corners=None, ids=None, camera=None, inlier_px=None, min_markers: int = 2):
        """The map pose by consensus on the markers of one frame handed in from the host (fid_map_pose_robust_cam): the pose from
        the largest set of markers that agree within inlier_px pixels, and which markers were left out.  Returns one
        MAP_POSE_DTYPE record and one MAP_ROBUST_DTYPE record; map_robust_outlier_ids turns the latter into ids."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        opts = self._robust_opts(inlier_px, min_markers)
        ids = np.asarray(ids, np.int32).reshape(-1)
        mk = np.zeros(len(ids), _MARKER_DT)
        mk["id"] = ids
        mk["corners"] = np.asarray(corners, np.float32).reshape(len(ids), 8)
        out = np.zeros(1, MAP_POSE_DTYPE)
        rob = np.zeros(1, MAP_ROBUST_DTYPE)
        self._check(self._L.fid_map_pose_robust_cam(self._ctx, C.byref(cam.c), mk.ctypes.data if len(mk) else None, len(mk), C.byref(opts),
                                                    out.ctypes.data, rob.ctypes.data))
        return out[0], rob[0]

    def map_pose_robust_last(self, K=None, D=None, camera=None, inlier_px=None, min_markers: int = 2):
        """map_pose_robust for every frame of the last detect_* / collect call, on the markers where they lie
        (fid_map_pose_robust_last_cam): (MAP_POSE_DTYPE records, MAP_ROBUST_DTYPE records), one of each per frame."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        opts = self._robust_opts(inlier_px, min_markers)
        out = np.zeros(max(self._last_frames, 1), MAP_POSE_DTYPE)
        rob = np.zeros(len(out), MAP_ROBUST_DTYPE)
        self._check(self._L.fid_map_pose_robust_last_cam(self._ctx, C.byref(cam.c), C.byref(opts), out.ctypes.data, rob.ctypes.data, len(out)))
        return out[:self._last_frames], rob[:self._last_frames]

    # -- ChArUco boards ---------------------------------------------------------------------------
    def set_charuco_board(self, board) -> None:
        """The ChArUco board whose chessboard corners charuco_* interpolate (fid_set_charuco_board): a fiducials_amd.charuco.CharucoBoard;
        None clears it.  Independent of set_map."""
        if board is None:
            self._check(self._L.fid_set_charuco_board(self._ctx, None))
            self._charuco = None
            return
        b = board.c_struct()
        self._check(self._L.fid_set_charuco_board(self._ctx, C.byref(b)))
        self._charuco = board

    def _charuco_cap(self, cap):
        board = getattr(self, "_charuco", None)
        return int(cap) if cap is not None else (board.n_corners if board is not None else 1)

    def charuco_last(self, min_markers: int = 2, K=None, D=None, camera=None, cap: int | None = None) -> list:
        """The chessboard corners of every frame of the last detect_* / collect call, interpolated from its markers and refined on its
        gray frames without either leaving the device (fid_charuco_last_cam): a list of CHARUCO_CORNER_DTYPE arrays, one per frame, in
        ascending corner id.  Without a camera the positions come from the per-marker homographies; with K, D or camera= from the
        board pose and the camera's projection.  cap: the caller's room per frame (default: the board's corner count)."""
        cam = _camera.resolve(K, D, camera)
        cap = self._charuco_cap(cap)
        F = max(self._last_frames, 1)
        out = np.zeros(F * max(cap, 1), CHARUCO_CORNER_DTYPE)
        n = np.zeros(F, np.int32)
        self.last_charuco_counts = n
        self._check(self._L.fid_charuco_last_cam(self._ctx, C.byref(cam.c) if cam is not None else None, int(min_markers), out.ctypes.data, cap,
                                                 n.ctypes.data))
        return [out[f * cap:f * cap + int(n[f])].copy() for f in range(self._last_frames)]

    def charuco_interpolate(self, corners, ids, image, min_markers: int = 2, K=None, D=None, camera=None, cap: int | None = None) -> np.ndarray:
        """charuco_last's kernels on markers (corners (n, 4, 2), ids (n,), in list order) and a mono8 image from host memory
        (fid_charuco_interpolate_cam): one CHARUCO_CORNER_DTYPE array."""
        cam = _camera.resolve(K, D, camera)
        cap = self._charuco_cap(cap)
        ids = np.asarray(ids, np.int32).reshape(-1)
        mk = np.zeros(len(ids), _MARKER_DT)
        mk["id"] = ids
        mk["corners"] = np.asarray(corners, np.float32).reshape(len(ids), 8)
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise FidError(_lib.FID_E_INVALID_ARG, "charuco_interpolate takes a mono8 image (H, W) uint8")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        out = np.zeros(max(cap, 1), CHARUCO_CORNER_DTYPE)
        n = C.c_int32(0)
        self.last_charuco_counts = n
        self._check(self._L.fid_charuco_interpolate_cam(self._ctx, C.byref(cam.c) if cam is not None else None, mk.ctypes.data if len(mk) else None,
                                                        len(mk), img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], int(min_markers),
                                                        out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].copy()

    def charuco_pose(self, xy, ids, K=None, D=None, camera=None) -> np.ndarray:
        """estimatePoseCharucoBoard on corners handed in from the host (fid_charuco_pose_cam): xy (n, 2), ids (n,) chessboard corner
        indices.  Returns one CHARUCO_POSE_DTYPE record; status CHARUCO_POSE_* says why there is no pose."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        pts = np.ascontiguousarray(xy, dtype=np.float32).reshape(len(ids), 2)
        out = np.zeros(1, CHARUCO_POSE_DTYPE)
        self._check(self._L.fid_charuco_pose_cam(self._ctx, C.byref(cam.c), pts.ctypes.data if len(ids) else None, ids.ctypes.data if len(ids) else None,
                                                 len(ids), out.ctypes.data))
        return out[0]

    def charuco_pose_last(self, K=None, D=None, camera=None, min_markers: int = 2) -> np.ndarray:
        """The board pose of every frame of the last detect_* / collect call from its refined chessboard corners
        (fid_charuco_pose_last_cam: interpolation by the camera route, refinement, one solvePnP): CHARUCO_POSE_DTYPE records."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        out = np.zeros(max(self._last_frames, 1), CHARUCO_POSE_DTYPE)
        self._check(self._L.fid_charuco_pose_last_cam(self._ctx, C.byref(cam.c), int(min_markers), out.ctypes.data, len(out)))
        return out[:self._last_frames]

    # -- ChArUco diamonds -------------------------------------------------------------------------
    def _diamond_opts(self, square_marker_rate, max_rep_rate, refine):
        o = _lib.FidDiamondOpts()
        self._L.fid_default_diamond_opts(C.byref(o))
        if square_marker_rate is not None:
            o.square_marker_rate = float(square_marker_rate)
        if max_rep_rate is not None:
            o.max_rep_rate = float(max_rep_rate)
        o.refine = int(bool(refine))
        return o

    def diamonds_last(self, square_marker_rate: float | None = None, max_rep_rate: float | None = None, refine: bool = True,
                      cap: int = _lib.DIAMOND_MAX_PER_FRAME) -> list:
        """The diamonds (four markers around one chessboard square) among the markers of every frame of the last detect_* / collect
        call, their chessboard corners refined on its gray frames, nothing leaving the device in between (fid_diamonds_last): a list
        of DIAMOND_DTYPE arrays, one per frame, in the order of the diamonds' first markers.  square_marker_rate: square_len /
        marker_len of the print (default: marker_gen's sheet); max_rep_rate: the matching tolerance in marker sides (default 1.0:
        markers of about 30 px and more); cap: the caller's room per frame."""
        o = self._diamond_opts(square_marker_rate, max_rep_rate, refine)
        cap = int(cap)
        F = max(self._last_frames, 1)
        out = np.zeros(F * max(cap, 1), DIAMOND_DTYPE)
        n = np.zeros(F, np.int32)
        self.last_diamond_counts = n
        self._check(self._L.fid_diamonds_last(self._ctx, C.byref(o), out.ctypes.data, cap, n.ctypes.data))
        return [out[f * cap:f * cap + int(n[f])].copy() for f in range(self._last_frames)]

    def diamonds_detect(self, corners, ids, image, square_marker_rate: float | None = None, max_rep_rate: float | None = None,
                        refine: bool = True, cap: int = _lib.DIAMOND_MAX_PER_FRAME) -> np.ndarray:
        """diamonds_last's kernels on markers (corners (n, 4, 2), ids (n,), in list order) and a mono8 image from host memory
        (fid_diamonds_detect): one DIAMOND_DTYPE array."""
        o = self._diamond_opts(square_marker_rate, max_rep_rate, refine)
        cap = int(cap)
        ids = np.asarray(ids, np.int32).reshape(-1)
        mk = np.zeros(len(ids), _MARKER_DT)
        mk["id"] = ids
        mk["corners"] = np.asarray(corners, np.float32).reshape(len(ids), 8)
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise FidError(_lib.FID_E_INVALID_ARG, "diamonds_detect takes a mono8 image (H, W) uint8")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        out = np.zeros(max(cap, 1), DIAMOND_DTYPE)
        n = C.c_int32(0)
        self.last_diamond_counts = n
        self._check(self._L.fid_diamonds_detect(self._ctx, C.byref(o), mk.ctypes.data if len(mk) else None, len(mk), img.ctypes.data, img.shape[1],
                                                img.shape[0], img.strides[0], out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].copy()

    def diamond_pose(self, diamonds, square_len: float, K=None, D=None, camera=None) -> PoseResult:
        """The diamonds as fiducials of side square_len centred on their middle squares (fid_diamond_pose_cam: fid_pose_cam on
        {ids[0], corners}): DIAMOND_DTYPE records in, a PoseResult out."""
        cam = _camera.resolve(K, D, camera)
        if cam is None:
            raise ValueError("a pose needs K, D or camera=")
        d = np.ascontiguousarray(diamonds, dtype=DIAMOND_DTYPE).reshape(-1)
        out = (FidPoseOut * max(len(d), 1))()
        self._check(self._L.fid_diamond_pose_cam(self._ctx, C.byref(cam.c), d.ctypes.data if len(d) else None, len(d), float(square_len), out))
        return _poses_to_result(out, len(d))

    # -- calibration ------------------------------------------------------------------------------
    def _calib_setup(self, who, model, free, start, fix_aspect, max_iter, eps, min_items):
        """fid_calib_opts and the camera that goes in, as calibrate_map and calibrate_charuco both read their arguments."""
        default_free = {_lib.CAM_PLUMB_BOB: (_lib.CALIB_FREE_PLUMB_BOB, 5), _lib.CAM_RATIONAL: (_lib.CALIB_FREE_RATIONAL, 8),
                        _lib.CAM_EQUIDISTANT: (_lib.CALIB_FREE_EQUIDISTANT, 4)}
        opts = _lib.FidCalibOpts()
        self._L.fid_default_calib_opts(C.byref(opts))
        if start is None:
            if int(model) not in default_free:
                raise FidError(_lib.FID_E_INVALID_ARG, f"{who}: model {model} is not a CAM_* value")
            mask, nd = default_free[int(model)]
            if free is not None:
                mask = int(free)
                if int(model) == _lib.CAM_RATIONAL and mask >> 12:
                    nd = 12
            cam = _camera.Camera(int(model), np.eye(3), np.zeros(nd))
            opts.start = _lib.CALIB_START_AUTO
        else:
            if not isinstance(start, _camera.Camera):
                raise TypeError("start= takes a fiducials_amd.camera.Camera")
            cam = _camera.Camera(start.model, start.K, start.D)
            mask = default_free[cam.model][0] & ((1 << (4 + cam.n_dist)) - 1) if free is None else int(free)
            opts.start = _lib.CALIB_START_GIVEN
        opts.free_mask = mask
        opts.fix_aspect = 1 if fix_aspect else 0
        opts.min_markers = int(min_items)
        if max_iter is not None:
            opts.max_iter = int(max_iter)
        if eps is not None:
            opts.eps = float(eps)
        return opts, cam

    def calibrate_map(self, views, image_size, model: int = _lib.CAM_PLUMB_BOB, free: int | None = None, start=None, fix_aspect: bool = False,
                      max_iter: int | None = None, eps: float | None = None, min_markers: int = 1):
        """The camera from views of the context's map (fid_calibrate_map; set_map first).  views: a list of (corners (n, 4, 2), ids (n,))
        as detect_markers_batch returns them, or of (ids, corners).  image_size: (width, height).  model: CAM_*.  free: a CALIB_FREE_*
        mask (default: the model's usual one -- plumb-bob 9 slots, rational 12, equidistant 8).  start: None for the AUTO start (planar
        maps), or the Camera to start from -- it also gives the values of the slots that are not free and, with fix_aspect, the ratio
        fx / fy.  Returns (Camera, CALIB_OUT_DTYPE record, CALIB_VIEW_DTYPE array)."""
        L = self._L
        opts, cam = self._calib_setup("calibrate_map", model, free, start, fix_aspect, max_iter, eps, min_markers)
        # a view: (corners, ids) as detect_markers_batch returns it, or (ids, corners) -- the ids are the flat one of the pair
        views = [(a, b) if np.asarray(b).ndim <= 1 and np.asarray(a).ndim > 1 else (b, a) for a, b in views]
        cap = max([len(np.asarray(v[1]).reshape(-1)) for v in views] + [1])
        mk = np.zeros((max(len(views), 1), cap), _MARKER_DT)
        n = np.zeros(max(len(views), 1), np.int32)
        for i, (corners, ids) in enumerate(views):
            ids = np.asarray(ids, np.int32).reshape(-1)
            n[i] = len(ids)
            mk["id"][i, :len(ids)] = ids
            mk["corners"][i, :len(ids)] = np.asarray(corners, np.float32).reshape(len(ids), 8)
        out = np.zeros(1, _lib.CALIB_OUT_DTYPE)
        vout = np.zeros(max(len(views), 1), _lib.CALIB_VIEW_DTYPE)
        self._check(L.fid_calibrate_map(self._ctx, mk.ctypes.data, n.ctypes.data, len(views), cap, int(image_size[0]), int(image_size[1]), C.byref(opts),
                                        C.byref(cam.c), out.ctypes.data, vout.ctypes.data))
        return cam, out[0], vout[:len(views)]

    def calibrate_charuco(self, views, image_size, model: int = _lib.CAM_PLUMB_BOB, free: int | None = None, start=None, fix_aspect: bool = False,
                          max_iter: int | None = None, eps: float | None = None, min_points: int = 4):
        """The camera from views of the context's ChArUco board (fid_calibrate_charuco; set_charuco_board first).  views: the list
        charuco_last returns (one CHARUCO_CORNER_DTYPE array per frame), or a list of (ids (n,), xy (n, 2)) pairs.  Everything else is
        calibrate_map's; start=None is the AUTO start, which a board always allows.  min_points: a view with fewer used points (never
        fewer than four) is skipped.  Returns (Camera, CALIB_OUT_DTYPE record, CALIB_VIEW_DTYPE array)."""
        opts, cam = self._calib_setup("calibrate_charuco", model, free, start, fix_aspect, max_iter, eps, min_points)
        recs = []
        for view in views:
            if isinstance(view, np.ndarray) and view.dtype == CHARUCO_CORNER_DTYPE:
                recs.append(view.reshape(-1))
                continue
            ids, xy = view
            ids = np.asarray(ids, np.int32).reshape(-1)
            r = np.zeros(len(ids), CHARUCO_CORNER_DTYPE)
            r["id"] = ids
            r["x"], r["y"] = np.asarray(xy, np.float32).reshape(len(ids), 2).T
            r["x0"], r["y0"] = r["x"], r["y"]
            recs.append(r)
        cap = max([len(r) for r in recs] + [1])
        packed = np.zeros((max(len(recs), 1), cap), CHARUCO_CORNER_DTYPE)
        n = np.zeros(max(len(recs), 1), np.int32)
        for i, r in enumerate(recs):
            n[i] = len(r)
            packed[i, :len(r)] = r
        out = np.zeros(1, _lib.CALIB_OUT_DTYPE)
        vout = np.zeros(max(len(recs), 1), _lib.CALIB_VIEW_DTYPE)
        self._check(self._L.fid_calibrate_charuco(self._ctx, packed.ctypes.data, n.ctypes.data, len(recs), cap, int(image_size[0]), int(image_size[1]),
                                                  C.byref(opts), C.byref(cam.c), out.ctypes.data, vout.ctypes.data))
        return cam, out[0], vout[:len(recs)]

    # -- building the map -------------------------------------------------------------------------
    def build_map(self, views, camera, fiducial_len: float, fixed, len_override: dict | None = None, min_views: int = 2, max_iter: int | None = None,
                  eps: float | None = None, sigma_px: float = 0.0):
        """The map from a set of views by bundle adjustment on the device (fid_build_map_cam).  views: a list of (corners (n, 4, 2), ids
        (n,)) as detect_markers_batch returns them, or of (ids, corners).  camera: a Camera (or (K, D) for plumb-bob), the same for every
        view.  fixed: MAP_ENTRY_DTYPE records that define the map frame (at least one).  len_override: {id: length}.  Returns (entries,
        out, markers, views): entries (MAP_ENTRY_DTYPE, the FIXED and SOLVED markers) goes straight into set_map; out a BUILD_OUT_DTYPE
        record, markers a BUILD_MARKER_DTYPE array of every id seen, views a BUILD_VIEW_DTYPE array."""
        return self._build_map(None, views, camera, fiducial_len, fixed, len_override, min_views, max_iter, eps, sigma_px)

    def build_map_robust(self, views, camera, fiducial_len: float, fixed, inlier_px: float, min_views_place: int = 1, len_override: dict | None = None,
                         min_views: int = 2, max_iter: int | None = None, eps: float | None = None, sigma_px: float = 0.0):
        """build_map over views that hold wrong detections (fid_build_map_robust_cam): the solve is run in at most four rounds, each over
        the observations within inlier_px of the round before, from a start made by consensus.  inlier_px has no default; the header
        recommends _lib.BUILD_ROBUST_INLIER_PX.  Returns build_map's tuple plus (robust_out, obs_state, obs_err_px, marker_outliers,
        view_outliers): a BUILD_ROBUST_OUT_DTYPE record; per view a uint8 array of _lib.OBS_* and a float64 array of the errors (-1 where
        there is none), both parallel to the view's list; the outlier observations per entry of `markers` and per view (int32)."""
        return self._build_map((float(inlier_px), int(min_views_place)), views, camera, fiducial_len, fixed, len_override, min_views, max_iter, eps, sigma_px)

    def _build_map(self, robust, views, camera, fiducial_len, fixed, len_override, min_views, max_iter, eps, sigma_px):
        L = self._L
        cam = camera if isinstance(camera, _camera.Camera) else _camera.resolve(camera[0], camera[1], None)
        opts = _lib.FidBuildOpts()
        L.fid_default_build_opts(C.byref(opts))
        opts.fiducial_len = float(fiducial_len)
        opts.min_views = int(min_views)
        opts.sigma_px = float(sigma_px)
        if max_iter is not None:
            opts.max_iter = int(max_iter)
        if eps is not None:
            opts.eps = float(eps)
        lids = np.ascontiguousarray(list((len_override or {}).keys()), dtype=np.int32)
        lvals = np.ascontiguousarray(list((len_override or {}).values()), dtype=np.float64)
        if len(lids):
            opts.len_ids, opts.len_values, opts.n_len = lids.ctypes.data, lvals.ctypes.data, len(lids)
        fx = np.zeros(0, MAP_ENTRY_DTYPE) if fixed is None else np.ascontiguousarray(fixed, dtype=MAP_ENTRY_DTYPE).reshape(-1)
        views = [(a, b) if np.asarray(b).ndim <= 1 and np.asarray(a).ndim > 1 else (b, a) for a, b in views]
        cap = max([len(np.asarray(v[1]).reshape(-1)) for v in views] + [1])
        mk = np.zeros((max(len(views), 1), cap), _MARKER_DT)
        n = np.zeros(max(len(views), 1), np.int32)
        for i, (corners, ids) in enumerate(views):
            ids = np.asarray(ids, np.int32).reshape(-1)
            n[i] = len(ids)
            mk["id"][i, :len(ids)] = ids
            mk["corners"][i, :len(ids)] = np.asarray(corners, np.float32).reshape(len(ids), 8)
        out = np.zeros(1, _lib.BUILD_OUT_DTYPE)
        vout = np.zeros(max(len(views), 1), _lib.BUILD_VIEW_DTYPE)
        cap_m = max(int(n.sum()), 1)
        mout = np.zeros(cap_m, _lib.BUILD_MARKER_DTYPE)
        n_m = C.c_int32(0)
        if robust is None:
            self._check(L.fid_build_map_cam(self._ctx, C.byref(cam.c), mk.ctypes.data, n.ctypes.data, len(views), cap, fx.ctypes.data if len(fx) else None,
                                            len(fx), C.byref(opts), out.ctypes.data, mout.ctypes.data, cap_m, C.byref(n_m), vout.ctypes.data))
        else:
            ropts = _lib.FidBuildRobustOpts(robust[0], robust[1], 0)
            rout = np.zeros(1, _lib.BUILD_ROBUST_OUT_DTYPE)
            state = np.zeros((len(n), cap), np.uint8)
            err = np.zeros((len(n), cap), np.float64)
            m_outl = np.zeros(cap_m, np.int32)
            v_outl = np.zeros(len(n), np.int32)
            self._check(L.fid_build_map_robust_cam(self._ctx, C.byref(cam.c), mk.ctypes.data, n.ctypes.data, len(views), cap, fx.ctypes.data if len(fx) else None,
                                                   len(fx), C.byref(opts), C.byref(ropts), out.ctypes.data, rout.ctypes.data, mout.ctypes.data, cap_m, C.byref(n_m),
                                                   vout.ctypes.data, state.ctypes.data, err.ctypes.data, m_outl.ctypes.data, v_outl.ctypes.data))
        mout = mout[:n_m.value]
        ok = (mout["status"] == _lib.BUILD_MARKER_FIXED) | (mout["status"] == _lib.BUILD_MARKER_SOLVED)
        plain = (np.ascontiguousarray(mout["entry"][ok]).astype(MAP_ENTRY_DTYPE), out[0], mout, vout[:len(views)])
        if robust is None:
            return plain
        return plain + (rout[0], [state[v, :n[v]].copy() for v in range(len(views))], [err[v, :n[v]].copy() for v in range(len(views))], m_outl[:n_m.value],
                        v_outl[:len(views)])

    @staticmethod
    def save_map(path: str, markers) -> None:
        """build_map's markers as the file fiducial_slam reads as its map_file (the module's save_map)."""
        save_map(path, markers)

    # -- stage taps for parity tests ------------------------------------------------------------
    def tap(self, which: int) -> np.ndarray:
        nbytes = self._L.fid_tap_bytes(self._ctx, which)
        buf = np.zeros(nbytes, dtype=np.uint8)
        self._check(self._L.fid_tap_read(self._ctx, which, buf.ctypes.data, nbytes))
        return buf

    def tap_counts(self):
        return self.tap(_lib.TAP_COUNTS).view(np.int32).reshape(-1, 12)

    def tap_masks(self, nframes, nscales, h, w):
        ww = (w + 31) // 32
        m = self.tap(_lib.TAP_MASKS).view(np.uint32).reshape(nframes, nscales, h, ww)
        bits = np.unpackbits(m.view(np.uint8).reshape(nframes, nscales, h, ww * 4), axis=-1, bitorder="little")
        return bits[..., :w]

    def tap_candidates(self, filtered: bool = False):
        raw = self.tap(_lib.TAP_FILTERED if filtered else _lib.TAP_CANDIDATES)
        dt = np.dtype([("scale", "<i4"), ("contour_size", "<i4"), ("start_x", "<i4"), ("start_y", "<i4"),
                       ("is_hole", "<i4"), ("corners", "<f4", (8,))])
        return raw.view(dt).reshape(-1, self.limits.max_candidates_per_frame)

    def tap_bits(self):
        msb = self.dictionary.marker_size + 2 * self.params.markerBorderBits
        return self.tap(_lib.TAP_BITS).reshape(-1, self.limits.max_candidates_per_frame, msb, msb)

    def tap_ident(self):
        return self.tap(_lib.TAP_IDENT).view(np.int32).reshape(-1, self.limits.max_candidates_per_frame, 2)

    def tap_presubpix(self):
        dt = np.dtype([("id", "<i4"), ("corners", "<f4", (8,))])
        return self.tap(_lib.TAP_PRESUBPIX).view(dt).reshape(-1, self.max_markers)

    def stage_ms(self) -> dict:
        ms = (C.c_float * 32)()
        names = C.POINTER(C.c_char_p)()
        n = self._L.fid_last_stage_ms(self._ctx, ms, 32, C.byref(names))
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    def last_launches(self) -> int:
        """Launches per kernel in the last detect call (sub-batches on separate streams)."""
        return int(self._L.fid_last_launches(self._ctx))

    @property
    def stream(self) -> int:
        return int(self._L.fid_stream(self._ctx) or 0)
