"""ctypes binding of the C-ABI (include/fid_abi.h).  Loading fails loudly if the HIP library is missing:
there is no CPU fallback in this package."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build


class FidParams(C.Structure):
    _fields_ = [
        ("adaptiveThreshConstant", C.c_double),
        ("adaptiveThreshWinSizeMin", C.c_int32),
        ("adaptiveThreshWinSizeMax", C.c_int32),
        ("adaptiveThreshWinSizeStep", C.c_int32),
        ("cornerRefinementMethod", C.c_int32),
        ("cornerRefinementWinSize", C.c_int32),
        ("cornerRefinementMaxIterations", C.c_int32),
        ("cornerRefinementMinAccuracy", C.c_double),
        ("errorCorrectionRate", C.c_double),
        ("minCornerDistanceRate", C.c_double),
        ("markerBorderBits", C.c_int32),
        ("minDistanceToBorder", C.c_int32),
        ("maxErroneousBitsInBorderRate", C.c_double),
        ("minMarkerDistanceRate", C.c_double),
        ("minMarkerPerimeterRate", C.c_double),
        ("maxMarkerPerimeterRate", C.c_double),
        ("minOtsuStdDev", C.c_double),
        ("perspectiveRemoveIgnoredMarginPerCell", C.c_double),
        ("perspectiveRemovePixelPerCell", C.c_int32),
        ("reserved0", C.c_int32),
        ("polygonalApproxAccuracyRate", C.c_double),
    ]


class FidDict(C.Structure):
    _fields_ = [("marker_size", C.c_int32), ("max_correction_bits", C.c_int32), ("n_markers", C.c_int32),
                ("reserved0", C.c_int32), ("bytes", C.c_void_p)]


class FidMarker(C.Structure):
    _fields_ = [("id", C.c_int32), ("corners", C.c_float * 8)]


class FidPoseOut(C.Structure):
    _fields_ = [("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("image_error", C.c_double),
                ("object_error", C.c_double), ("fiducial_area", C.c_double)]


class FidMapEntry(C.Structure):
    _fields_ = [("id", C.c_int32), ("reserved0", C.c_int32), ("len", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3)]


class FidMapPoseOut(C.Structure):
    _fields_ = [("n_markers", C.c_int32), ("n_over", C.c_int32), ("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("R", C.c_double * 9),
                ("cam_R", C.c_double * 9), ("cam_t", C.c_double * 3), ("image_error", C.c_double)]


class FidCamera(C.Structure):
    """fid_camera: the camera as a value -- model (CAM_*), the number of coefficients given, K row-major, D (zero beyond n_dist)."""
    _fields_ = [("model", C.c_int32), ("n_dist", C.c_int32), ("K", C.c_double * 9), ("D", C.c_double * 12)]


class FidRigCamera(C.Structure):
    """fid_rig_camera: a camera of a rig -- the camera and the rig frame in the camera frame, X_cam = R X_rig + t."""
    _fields_ = [("cam", FidCamera), ("R", C.c_double * 9), ("t", C.c_double * 3)]


class FidMapRobustOpts(C.Structure):
    """fid_map_robust_opts: inlier_px (finite, > 0), min_markers (>= 1)."""
    _fields_ = [("inlier_px", C.c_double), ("min_markers", C.c_int32), ("reserved0", C.c_int32)]


class FidBuildOpts(C.Structure):
    """fid_build_opts (fid_default_build_opts fills the defaults)."""
    _fields_ = [("fiducial_len", C.c_double), ("len_ids", C.c_void_p), ("len_values", C.c_void_p), ("n_len", C.c_int32), ("min_views", C.c_int32),
                ("max_iter", C.c_int32), ("reserved0", C.c_int32), ("eps", C.c_double), ("sigma_px", C.c_double)]


class FidBuildRobustOpts(C.Structure):
    """fid_build_robust_opts: inlier_px (finite, > 0, no default), min_views_place (>= 1)."""
    _fields_ = [("inlier_px", C.c_double), ("min_views_place", C.c_int32), ("reserved0", C.c_int32)]


class FidCalibOpts(C.Structure):
    """fid_calib_opts (fid_default_calib_opts fills the defaults)."""
    _fields_ = [("free_mask", C.c_uint32), ("start", C.c_int32), ("fix_aspect", C.c_int32), ("min_markers", C.c_int32), ("max_iter", C.c_int32),
                ("reserved0", C.c_int32), ("eps", C.c_double)]


class FidDiamondOpts(C.Structure):
    """fid_diamond_opts: square_len / marker_len, the matching tolerance in marker sides, whether to refine."""
    _fields_ = [("square_marker_rate", C.c_double), ("max_rep_rate", C.c_double), ("refine", C.c_int32), ("reserved0", C.c_int32)]


class FidCharucoBoard(C.Structure):
    """fid_charuco_board: squares a side, square and marker length, the id of the first marker."""
    _fields_ = [("squares_x", C.c_int32), ("squares_y", C.c_int32), ("square_len", C.c_double), ("marker_len", C.c_double), ("first_id", C.c_int32),
                ("reserved0", C.c_int32)]


class FidLimits(C.Structure):
    _fields_ = [("max_width", C.c_int32), ("max_height", C.c_int32), ("max_batch", C.c_int32),
                ("max_starts_per_frame", C.c_int32), ("max_contours_per_frame", C.c_int32),
                ("max_candidates_per_frame", C.c_int32), ("max_markers_per_frame", C.c_int32),
                ("max_points_per_frame", C.c_int32)]


class FidCandidate(C.Structure):
    _fields_ = [("scale", C.c_int32), ("contour_size", C.c_int32), ("start_x", C.c_int32), ("start_y", C.c_int32),
                ("is_hole", C.c_int32), ("corners", C.c_float * 8)]


class FidJpegInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("h_samp", C.c_int32), ("v_samp", C.c_int32),
                ("restart_interval", C.c_int32), ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3), ("scan_bytes", C.c_int64)]


class FidPngInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32), ("interlace", C.c_int32),
                ("gray", C.c_int32)]


FID_OK = 0
FID_E_INVALID_ARG, FID_E_NO_DEVICE, FID_E_HIP, FID_E_CAPACITY, FID_E_OUT_OF_MEMORY, FID_E_UNSUPPORTED, FID_E_CV_EXCEPTION = 1, 2, 3, 4, 5, 6, 7
CORNER_REFINE_NONE, CORNER_REFINE_SUBPIX, CORNER_REFINE_CONTOUR = 0, 1, 2  # aruco::CornerRefineMethod as the node sets it (:700-711)
ENC = {"mono8": 0, "bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4,
       # ABI 7: what raw camera drivers publish, converted on the device (fid_encoding in include/fid_abi.h)
       "bayer_rggb8": 5, "bayer_bggr8": 6, "bayer_gbrg8": 7, "bayer_grbg8": 8, "mono16": 9, "bgr16": 10, "rgb16": 11, "bgra16": 12, "rgba16": 13,
       "yuv422": 14}
ENC_BIGENDIAN = 0x100  # OR-ed onto a 16-bit encoding (sensor_msgs/Image.is_bigendian)
ENC_BYTES_PER_PIXEL = {"mono8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "bayer_rggb8": 1, "bayer_bggr8": 1, "bayer_gbrg8": 1,
                       "bayer_grbg8": 1, "mono16": 2, "bgr16": 6, "rgb16": 6, "bgra16": 8, "rgba16": 8, "yuv422": 2}


def encoding_value(encoding: str, is_bigendian: bool = False) -> int:
    """fid_encoding of a sensor_msgs/Image encoding string (the table fid_encoding_from_string holds)."""
    v = ENC[encoding]
    return v | ENC_BIGENDIAN if is_bigendian and 9 <= v <= 13 else v


CAM_PLUMB_BOB, CAM_RATIONAL, CAM_EQUIDISTANT = 0, 1, 2  # fid_camera_model
# fid_pose_cov / fid_map_pose_cov as numpy records (status 0: valid, 1: no pose, 2: J^T J not positive definite; cov_pose in
# geometry_msgs/PoseWithCovariance order)
POSE_COV_FIELDS = [("status", "<i4"), ("n_points", "<i4"), ("sigma2", "<f8"), ("cov_rt", "<f8", (6, 6)), ("cov_pose", "<f8", (6, 6))]
MAP_MAX_ENTRIES, MAP_MAX_USED = 4096, 256  # FID_MAP_MAX_ENTRIES, FID_MAP_MAX_USED
# fid_map_robust_out as a numpy record (fid_abi.h: "map pose that survives wrong markers"); status: MAP_ROBUST_*
MAP_ROBUST_OK, MAP_ROBUST_NO_CONSENSUS, MAP_ROBUST_NO_MARKERS = 0, 1, 2
MAP_ROBUST_HYPOTHESES, MAP_ROBUST_SOLVES = 64, 4  # FID_MAP_ROBUST_HYPOTHESES, FID_MAP_ROBUST_SOLVES
MAP_ROBUST_INLIER_PX = 4.0  # the header's RECOMMENDED inlier_px (the ABI has no default)
MAP_ROBUST_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("n_inliers", "<i4"), ("n_outliers", "<i4"), ("hypothesis", "<i4"),
                             ("rounds", "<i4"), ("stable", "<i4"), ("reserved0", "<i4"), ("score", "<f8"), ("worst_inlier_px", "<f8"),
                             ("best_outlier_px", "<f8"), ("outlier_mask", "<u8", (4,)), ("outlier_index", "<i4", (16,))])
# fid_calibrate_map (fid_abi.h: "camera calibration from views of the map")
CALIB_MAX_VIEWS = 1024
CALIB_START_GIVEN, CALIB_START_AUTO = 0, 1
CALIB_OK, CALIB_MAX_ITER, CALIB_STALLED = 0, 1, 2
CALIB_VIEW_USED, CALIB_VIEW_FEW, CALIB_VIEW_NO_START = 0, 1, 2
CALIB_FREE_FOCAL, CALIB_FREE_K, CALIB_FREE_PLUMB_BOB, CALIB_FREE_PLUMB_BOB_NO_K3 = 0x0003, 0x000F, 0x01FF, 0x00FF
CALIB_FREE_EQUIDISTANT, CALIB_FREE_RATIONAL, CALIB_FREE_RATIONAL_PRISM = 0x00FF, 0x0FFF, 0xFFFF
CALIB_OUT_DTYPE = np.dtype([("status", "<i4"), ("n_views_used", "<i4"), ("n_points", "<i4"), ("n_iter", "<i4"), ("n_free", "<i4"), ("reserved0", "<i4"),
                            ("cost", "<f8"), ("rms", "<f8"), ("start_cost", "<f8"), ("std_dev", "<f8", (16,))])  # fid_calib_out
CALIB_VIEW_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("n_over", "<i4"), ("reserved0", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)),
                             ("rms", "<f8")])  # fid_calib_view
# fid_build_map_cam (fid_abi.h: "building the map"); status: BUILD_*, a marker's: BUILD_MARKER_*, a view's: BUILD_VIEW_*
BUILD_MAX_VIEWS, BUILD_MAX_MARKERS, BUILD_MAX_PER_VIEW = 4096, 128, 64
BUILD_OK, BUILD_MAX_ITER, BUILD_STALLED = 0, 1, 2
BUILD_MARKER_FIXED, BUILD_MARKER_SOLVED, BUILD_MARKER_FEW_VIEWS, BUILD_MARKER_UNREACHED, BUILD_MARKER_NO_START = 0, 1, 2, 3, 4
BUILD_VIEW_USED, BUILD_VIEW_FEW, BUILD_VIEW_UNREACHED, BUILD_VIEW_NO_START = 0, 1, 2, 3
BUILD_OUT_DTYPE = np.dtype([("status", "<i4"), ("n_views_used", "<i4"), ("n_markers", "<i4"), ("n_fixed", "<i4"), ("n_points", "<i4"), ("n_iter", "<i4"),
                            ("n_free", "<i4"), ("reserved0", "<i4"), ("cost", "<f8"), ("start_cost", "<f8"), ("rms", "<f8")])  # fid_build_out
_MAP_ENTRY_DT = np.dtype([("id", "<i4"), ("reserved0", "<i4"), ("len", "<f8"), ("R", "<f8", (3, 3)), ("t", "<f8", (3,))])  # fid_map_entry
BUILD_MARKER_DTYPE = np.dtype([("id", "<i4"), ("status", "<i4"), ("n_views", "<i4"), ("slot", "<i4"), ("links", "<u4", (4,)), ("rms", "<f8"),
                               ("entry", _MAP_ENTRY_DT), ("cov", "<f8", (6, 6))])  # fid_build_marker
BUILD_VIEW_DTYPE = np.dtype([("status", "<i4"), ("n_used", "<i4"), ("n_over", "<i4"), ("reserved0", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)),
                             ("rms", "<f8")])  # fid_build_view
# fid_build_map_robust_cam (fid_abi.h: "building the map from views that hold wrong detections"); an observation's state: OBS_*
BUILD_ROBUST_SOLVES, BUILD_ROBUST_HYPOTHESES = 4, 64
OBS_NOT_KEPT, OBS_INLIER, OBS_OUTLIER, OBS_LEFT_OUT = 0, 1, 2, 3
BUILD_ROBUST_MEASURED_PX, BUILD_ROBUST_INLIER_PX = 1.3215, 13.5  # the header's measured err and RECOMMENDED inlier_px (the ABI has no default)
BUILD_ROBUST_OUT_DTYPE = np.dtype([("rounds", "<i4"), ("stable", "<i4"), ("n_obs", "<i4"), ("n_inliers", "<i4"), ("n_outliers", "<i4"), ("reserved0", "<i4"),
                                   ("worst_inlier_px", "<f8"), ("best_outlier_px", "<f8")])  # fid_build_robust_out
# ChArUco boards (fid_abi.h: "ChArUco boards"); a pose record's status: CHARUCO_POSE_*
CHARUCO_MAX_SQUARES = 512  # FID_CHARUCO_MAX_SQUARES
CHARUCO_POSE_OK, CHARUCO_POSE_FEW, CHARUCO_POSE_COLLINEAR, CHARUCO_POSE_VOID = 0, 1, 2, 3
CHARUCO_CORNER_DTYPE = np.dtype([("id", "<i4"), ("win", "<i4"), ("x", "<f4"), ("y", "<f4"), ("x0", "<f4"), ("y0", "<f4")])  # fid_charuco_corner
CHARUCO_POSE_DTYPE = np.dtype([("n_corners", "<i4"), ("status", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("R", "<f8", (3, 3)),
                               ("cam_R", "<f8", (3, 3)), ("cam_t", "<f8", (3,)), ("image_error", "<f8")])  # fid_charuco_pose_out
# ChArUco diamonds (fid_abi.h: "ChArUco diamonds")
DIAMOND_MAX_PER_FRAME, DIAMOND_MAX_MARKERS = 64, 256  # FID_DIAMOND_MAX_PER_FRAME, FID_DIAMOND_MAX_MARKERS
DIAMOND_DTYPE = np.dtype([("ids", "<i4", (4,)), ("index", "<i4", (4,)), ("corners", "<f4", (4, 2)), ("corners0", "<f4", (4, 2)),
                          ("win", "<i4", (4,))])  # fid_diamond
# the camera rig (fid_abi.h: "one rig pose per time step")
RIG_MAX_CAMERAS, RIG_MAX_USED = 16, 128  # FID_RIG_MAX_CAMERAS, FID_RIG_MAX_USED
RIG_POSE_DTYPE = np.dtype([("n_markers", "<i4"), ("n_cameras", "<i4"), ("n_over", "<i4"), ("n_unposable", "<i4"), ("start_camera", "<i4"),
                           ("n_per_camera", "<i4", (RIG_MAX_CAMERAS,)), ("reserved0", "<i4"), ("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("R", "<f8", (3, 3)),
                           ("rig_R", "<f8", (3, 3)), ("rig_t", "<f8", (3,)), ("image_error", "<f8"), ("err_per_camera", "<f8", (RIG_MAX_CAMERAS,))],
                          )  # fid_rig_pose_out: 22 int32, then doubles -- no padding
assert RIG_POSE_DTYPE.itemsize == 440 and RIG_POSE_DTYPE.fields["rvec"][1] == 88
TAP_MASKS, TAP_CANDIDATES, TAP_FILTERED, TAP_BITS, TAP_IDENT, TAP_PRESUBPIX, TAP_COUNTS, TAP_GRAY = range(8)

# every symbol include/fid_abi.h declares
SYMBOLS = [
    "fid_default_params", "fid_default_limits", "fid_create", "fid_destroy", "fid_set_params", "fid_detect",
    "fid_detect_batch", "fid_detect_device", "fid_submit_device", "fid_submit_batch", "fid_collect", "fid_order_after", "fid_pose", "fid_pose_last", "fid_refine_contour_corners", "fid_tap_bytes", "fid_tap_read",
    "fid_last_stage_ms", "fid_last_launches", "fid_stream", "fid_strerror", "fid_last_error", "fid_abi_version",
    "fid_stag_create", "fid_stag_destroy", "fid_stag_edge_frontend", "fid_stag_detect_edges", "fid_stag_detect_edges_validated", "fid_stag_detect_lines", "fid_stag_detect_lines_validated", "fid_stag_detect_quads", "fid_stag_host_tables", "fid_stag_load_library", "fid_stag_detect_markers_unrefined", "fid_stag_detect_markers", "fid_stag_pose_last", "fid_stag_detect_markers_batch", "fid_stag_tap_bytes", "fid_stag_tap_read", "fid_stag_queue_stats", "fid_stag_detect_markers_device", "fid_stag_detect_markers_batch_device",
    "fid_stag_tag_from_three_corners", "fid_stag_layout_load_file", "fid_stag_layout_last_error", "fid_stag_set_layout", "fid_stag_bundle_pose_last", "fid_stag_bundle_pose", "fid_stag_detect_bundles_batch", "fid_stag_detect_bundles_batch_device",
    "fid_map_load_file", "fid_map_last_error", "fid_map_entry_from_rpy", "fid_set_map", "fid_map_pose_last", "fid_map_pose",
    "fid_camera_from_info", "fid_camera_last_error", "fid_pose_cam", "fid_pose_last_cam", "fid_map_pose_last_cam", "fid_map_pose_cam", "fid_project_points_cam",
    "fid_stag_pose_last_cam", "fid_stag_detect_markers_batch_cam", "fid_stag_detect_markers_batch_device_cam", "fid_stag_bundle_pose_last_cam",
    "fid_stag_bundle_pose_cam", "fid_stag_detect_bundles_batch_cam", "fid_stag_detect_bundles_batch_device_cam",
    "fid_pose_cov_cam", "fid_pose_last_cov_cam", "fid_map_pose_last_cov_cam", "fid_map_pose_cov_cam",
    "fid_map_pose_robust_cam", "fid_map_pose_robust_last_cam",
    "fid_default_calib_opts", "fid_calibrate_map", "fid_camera_to_info", "fid_default_build_opts", "fid_build_map_cam", "fid_map_save_file",
    "fid_build_map_robust_cam",
    "fid_set_charuco_board", "fid_charuco_last_cam", "fid_charuco_interpolate_cam", "fid_charuco_pose_last_cam", "fid_charuco_pose_cam",
    "fid_calibrate_charuco",
    "fid_default_diamond_opts", "fid_diamonds_last", "fid_diamonds_detect", "fid_diamond_pose_cam",
    "fid_rig_camera_from_tf", "fid_set_rig", "fid_rig_steps_last", "fid_rig_pose_last", "fid_rig_pose",
    "fid_stag_pose_last_cov_cam", "fid_stag_bundle_pose_last_cov_cam", "fid_stag_bundle_pose_cov_cam",
    "fid_jpeg_probe", "fid_jpeg_create", "fid_jpeg_destroy", "fid_jpeg_decode", "fid_jpeg_device_ptr", "fid_jpeg_tap_bytes", "fid_jpeg_tap_read",
    "fid_jpeg_last_rounds", "fid_jpeg_last_error",
    "fid_png_probe", "fid_png_decode", "fid_png_last_error",
    "fid_to_bgr", "fid_image_to_bgr8", "fid_encoding_from_string", "fid_draw_detected_markers", "fid_dict_load_file", "fid_dict_last_error",
    "fid_to_bgr_device", "fid_draw_detected_markers_device", "fid_jpeg_marker_image",
    "fid_jpeg_enc_create", "fid_jpeg_enc_destroy", "fid_jpeg_enc_last_error", "fid_jpeg_enc_set", "fid_jpeg_encode_device", "fid_jpeg_encode",
    "fid_jpeg_enc_header", "fid_jpeg_marker_jpeg", "fid_jpeg_enc_tap_bytes", "fid_jpeg_enc_tap_read", "fid_jpeg_enc_last_ms",
]

_LIB = None


class FidError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"fid status {status}: {msg}")
        self.status = status


class CvException(FidError):
    """FID_E_CV_EXCEPTION: the input on which the reference's OpenCV call throws cv::Exception (the node's imageCallback logs
    it and publishes nothing for the frame, aruco_detect.cpp:391-393)."""


def device_text_sha256(path: str | None = None) -> str | None:
    """sha256 of the gfx950 code object's .text inside the library (ELF -> .hip_fatbin -> clang offload bundle -> the gfx950 ELF ->
    .text), in plain Python.  What the counter files under profiles/ are keyed to since round 5: a rebuild of the same sources
    changes the bundle's metadata (and so the file's hash) but not a byte of device code, and a change on the HOST side of the
    library (fid_draw.hip, the parsers) does not make the device counters stale.  None if the file cannot be read that way."""
    import hashlib
    import struct

    try:
        with open(path or lib_path(), "rb") as fh:
            b = fh.read()

        def sections(e):
            shoff = struct.unpack_from("<Q", e, 0x28)[0]
            es, sn, sx = struct.unpack_from("<HHH", e, 0x3A)
            hs = [struct.unpack_from("<IIQQQQ", e, shoff + i * es) for i in range(sn)]
            so = hs[sx][4]
            return {e[so + h[0]:e.index(b"\0", so + h[0])].decode(): (h[4], h[5]) for h in hs}

        off, size = sections(b)[".hip_fatbin"]
        f = b[off:off + size]
        if f[:24] != b"__CLANG_OFFLOAD_BUNDLE__":
            return None
        n = struct.unpack_from("<Q", f, 24)[0]
        p = 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", f, p)
            p += 24
            triple = f[p:p + tl].decode()
            p += tl
            if "gfx950" in triple:
                co = f[o:o + sz]
                to, ts = sections(co)[".text"]
                return hashlib.sha256(co[to:to + ts]).hexdigest()
    except Exception:  # noqa: BLE001
        return None
    return None


def profile_matches(doc: dict, path: str | None = None) -> bool:
    """Is a counter file under profiles/ (keyed to `device_text_sha256`, older ones to `library_sha256`) about THIS library?"""
    import hashlib

    dev = doc.get("device_text_sha256")
    if dev:
        return dev == device_text_sha256(path)
    try:
        with open(path or lib_path(), "rb") as fh:
            return hashlib.sha256(fh.read()).hexdigest() == doc.get("library_sha256")
    except OSError:
        return False


def lib_path() -> str:
    # FID_LIB lets a developer point at an instrumented build (e.g. -DFID_DEBUG_STATS); it is still libfid_amd
    return os.environ.get("FID_LIB") or _build.LIB


def load():
    """Load libfid_amd.so.  Raises if it has not been built (run `python -m fiducials_amd.build` or
    __graft_entry__.build()); never substitutes another implementation."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise FidError(FID_E_NO_DEVICE, f"{path} is missing: build the HIP library first (fiducials_amd.build.build())")
    L = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.fid_default_params.argtypes = [C.POINTER(FidParams)]
    L.fid_default_limits.argtypes = [C.POINTER(FidLimits)]
    L.fid_create.argtypes = [C.POINTER(FidParams), C.POINTER(FidDict), C.POINTER(FidLimits), C.c_int, C.POINTER(vp)]
    L.fid_destroy.argtypes = [vp]
    L.fid_destroy.restype = None
    L.fid_set_params.argtypes = [vp, C.POINTER(FidParams)]
    L.fid_detect.argtypes = [vp, vp, i32, i32, i32, C.c_int, C.POINTER(FidMarker), i32, C.POINTER(i32)]
    L.fid_detect_batch.argtypes = [vp, vp, i32, i32, i32, i32, i64, C.c_int, C.POINTER(FidMarker), i32, C.POINTER(i32)]
    L.fid_detect_device.argtypes = [vp, vp, i32, i32, i32, i32, i64, C.c_int, C.POINTER(FidMarker), i32, C.POINTER(i32)]
    L.fid_submit_device.argtypes = [vp, vp, i32, i32, i32, i32, i64, C.c_int]
    L.fid_submit_batch.argtypes = [vp, vp, i32, i32, i32, i32, i64, C.c_int]
    L.fid_collect.argtypes = [vp, C.POINTER(FidMarker), i32, C.POINTER(i32)]
    L.fid_order_after.argtypes = [vp, vp]
    L.fid_pose.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(FidMarker), C.POINTER(C.c_double),
                           i32, C.c_double, C.POINTER(FidPoseOut)]
    L.fid_pose_last.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(FidPoseOut), i32]
    L.fid_refine_contour_corners.argtypes = [vp, vp, vp, i32, vp, vp]
    L.fid_tap_bytes.argtypes = [vp, C.c_int]
    L.fid_tap_bytes.restype = i64
    L.fid_tap_read.argtypes = [vp, C.c_int, vp, i64]
    L.fid_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float), i32, C.POINTER(C.POINTER(C.c_char_p))]
    L.fid_last_stage_ms.restype = i32
    L.fid_last_launches.argtypes = [vp]
    L.fid_last_launches.restype = i32
    L.fid_stream.argtypes = [vp]
    L.fid_stream.restype = vp
    L.fid_strerror.argtypes = [C.c_int]
    L.fid_strerror.restype = C.c_char_p
    L.fid_last_error.argtypes = [vp]
    L.fid_last_error.restype = C.c_char_p
    L.fid_abi_version.restype = i32
    L.fid_stag_create.argtypes = [i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.fid_stag_destroy.argtypes = [vp]
    L.fid_stag_destroy.restype = None
    L.fid_stag_edge_frontend.argtypes = [vp, vp, i32, i32, i32]
    L.fid_stag_detect_edges.argtypes = [vp, vp, i32, i32, i32]
    L.fid_stag_detect_edges_validated.argtypes = [vp, vp, i32, i32, i32]
    L.fid_stag_detect_lines.argtypes = [vp, vp, i32, i32, i32]
    L.fid_stag_detect_lines_validated.argtypes = [vp, vp, i32, i32, i32]
    L.fid_stag_detect_quads.argtypes = [vp, vp, i32, i32, i32]
    L.fid_stag_load_library.argtypes = [vp, vp, i32]
    L.fid_stag_host_tables.argtypes = [i32, i32, vp, i32, vp, vp, vp, vp]
    L.fid_stag_detect_markers_unrefined.argtypes = [vp, vp, i32, i32, i32]
    L.fid_stag_detect_markers.argtypes = [vp, vp, i32, i32, i32, vp, i32, C.POINTER(i32)]
    L.fid_stag_pose_last.argtypes = [vp, vp, vp, C.c_double, vp, i32, C.POINTER(i32)]
    L.fid_stag_detect_markers_batch.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, vp, vp, C.c_double, vp, vp, i32, vp]
    L.fid_stag_tap_bytes.argtypes = [vp, C.c_int]
    L.fid_stag_tap_bytes.restype = i64
    L.fid_stag_tap_read.argtypes = [vp, C.c_int, vp, i64]
    L.fid_stag_queue_stats.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.fid_stag_detect_markers_device.argtypes = [vp, vp, i32, i32, i32, C.c_int, vp, i32, C.POINTER(i32)]
    L.fid_stag_detect_markers_batch_device.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, C.c_int, vp, vp, C.c_double, vp, vp, i32, vp]
    L.fid_stag_tag_from_three_corners.argtypes = [i32, i32, vp, vp, vp, vp]
    L.fid_stag_layout_load_file.argtypes = [C.c_char_p, vp, i32, C.POINTER(i32), C.POINTER(i32), vp, vp, i32]
    L.fid_stag_layout_last_error.argtypes = []
    L.fid_stag_layout_last_error.restype = C.c_char_p
    L.fid_stag_set_layout.argtypes = [vp, vp, i32, i32]
    L.fid_stag_bundle_pose_last.argtypes = [vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.fid_stag_bundle_pose.argtypes = [vp, vp, vp, vp, i32, vp, i32, C.POINTER(i32)]
    L.fid_stag_detect_bundles_batch.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, vp, vp, C.c_double, vp, vp, i32, vp, vp, vp]
    L.fid_stag_detect_bundles_batch_device.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, C.c_int, vp, vp, C.c_double, vp, vp, i32, vp, vp, vp]
    L.fid_map_load_file.argtypes = [C.c_char_p, C.c_double, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.fid_map_last_error.argtypes = []
    L.fid_map_last_error.restype = C.c_char_p
    L.fid_map_entry_from_rpy.argtypes = [i32, C.c_double, vp, vp, vp]
    L.fid_set_map.argtypes = [vp, vp, i32]
    L.fid_map_pose_last.argtypes = [vp, vp, vp, vp, i32]
    L.fid_map_pose.argtypes = [vp, vp, vp, vp, i32, vp]
    if hasattr(L, "fid_camera_from_info"):  # (the camera as a value; FID_LIB may name a build from before it)
        # the _cam twins: const fid_camera * in place of K[9], D[5]
        cam = C.POINTER(FidCamera)
        L.fid_camera_from_info.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), i32, cam]
        L.fid_camera_last_error.argtypes = []
        L.fid_camera_last_error.restype = C.c_char_p
        L.fid_pose_cam.argtypes = [vp, cam, C.POINTER(FidMarker), C.POINTER(C.c_double), i32, C.c_double, C.POINTER(FidPoseOut)]
        L.fid_pose_last_cam.argtypes = [vp, cam, C.c_double, C.POINTER(FidPoseOut), i32]
        L.fid_map_pose_last_cam.argtypes = [vp, cam, vp, i32]
        L.fid_map_pose_cam.argtypes = [vp, cam, vp, i32, vp]
        L.fid_project_points_cam.argtypes = [vp, cam, vp, vp, vp, i32, vp, vp]
        L.fid_stag_pose_last_cam.argtypes = [vp, cam, C.c_double, vp, i32, C.POINTER(i32)]
        L.fid_stag_detect_markers_batch_cam.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, cam, C.c_double, vp, vp, i32, vp]
        L.fid_stag_detect_markers_batch_device_cam.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, C.c_int, cam, C.c_double, vp, vp, i32, vp]
        L.fid_stag_bundle_pose_last_cam.argtypes = [vp, cam, vp, i32, C.POINTER(i32)]
        L.fid_stag_bundle_pose_cam.argtypes = [vp, cam, vp, i32, vp, i32, C.POINTER(i32)]
        L.fid_stag_detect_bundles_batch_cam.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, cam, C.c_double, vp, vp, i32, vp, vp, vp]
        L.fid_stag_detect_bundles_batch_device_cam.argtypes = [vp, i32, vp, i32, i32, i32, i32, i64, C.c_int, cam, C.c_double, vp, vp, i32, vp, vp, vp]
    if hasattr(L, "fid_pose_cov_cam"):  # (the pose covariance; FID_LIB may name a build from before it)
        cam = C.POINTER(FidCamera)
        L.fid_pose_cov_cam.argtypes = [vp, cam, C.POINTER(FidMarker), C.POINTER(C.c_double), i32, C.c_double, C.POINTER(FidPoseOut), C.c_double, vp]
        L.fid_pose_last_cov_cam.argtypes = [vp, cam, C.c_double, C.POINTER(FidPoseOut), i32, C.c_double, vp]
        L.fid_map_pose_last_cov_cam.argtypes = [vp, cam, vp, i32, C.c_double, vp]
        L.fid_map_pose_cov_cam.argtypes = [vp, cam, vp, i32, vp, C.c_double, vp]
        L.fid_stag_pose_last_cov_cam.argtypes = [vp, cam, C.c_double, vp, i32, C.POINTER(i32), C.c_double, vp]
        L.fid_stag_bundle_pose_last_cov_cam.argtypes = [vp, cam, vp, i32, C.POINTER(i32), C.c_double, vp]
        L.fid_stag_bundle_pose_cov_cam.argtypes = [vp, cam, vp, i32, vp, i32, C.POINTER(i32), C.c_double, vp]
    if hasattr(L, "fid_map_pose_robust_cam"):  # (the consensus map pose; FID_LIB may name a build from before it)
        cam = C.POINTER(FidCamera)
        L.fid_map_pose_robust_cam.argtypes = [vp, cam, vp, i32, C.POINTER(FidMapRobustOpts), vp, vp]
        L.fid_map_pose_robust_last_cam.argtypes = [vp, cam, C.POINTER(FidMapRobustOpts), vp, vp, i32]
    if hasattr(L, "fid_calibrate_map"):  # (calibration from views of the map; FID_LIB may name a build from before it)
        cam = C.POINTER(FidCamera)
        L.fid_default_calib_opts.argtypes = [C.POINTER(FidCalibOpts)]
        L.fid_default_calib_opts.restype = None
        L.fid_calibrate_map.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.POINTER(FidCalibOpts), cam, vp, vp]
        L.fid_camera_to_info.argtypes = [cam, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)]
    if hasattr(L, "fid_build_map_cam"):  # (building the map; FID_LIB may name a build from before it)
        L.fid_default_build_opts.argtypes = [C.POINTER(FidBuildOpts)]
        L.fid_default_build_opts.restype = None
        L.fid_build_map_cam.argtypes = [vp, C.POINTER(FidCamera), vp, vp, i32, i32, vp, i32, C.POINTER(FidBuildOpts), vp, vp, i32, C.POINTER(i32), vp]
        L.fid_map_save_file.argtypes = [C.c_char_p, vp, i32]
    if hasattr(L, "fid_build_map_robust_cam"):  # (the trimmed build; FID_LIB may name a build from before it)
        L.fid_build_map_robust_cam.argtypes = [vp, C.POINTER(FidCamera), vp, vp, i32, i32, vp, i32, C.POINTER(FidBuildOpts), C.POINTER(FidBuildRobustOpts), vp, vp,
                                               vp, i32, C.POINTER(i32), vp, vp, vp, vp, vp]
    if hasattr(L, "fid_set_charuco_board"):  # (ChArUco boards; FID_LIB may name a build from before them)
        cam = C.POINTER(FidCamera)
        L.fid_set_charuco_board.argtypes = [vp, C.POINTER(FidCharucoBoard)]
        L.fid_charuco_last_cam.argtypes = [vp, cam, i32, vp, i32, vp]
        L.fid_charuco_interpolate_cam.argtypes = [vp, cam, vp, i32, vp, i32, i32, i32, i32, vp, i32, C.POINTER(i32)]
        L.fid_charuco_pose_last_cam.argtypes = [vp, cam, i32, vp, i32]
        L.fid_charuco_pose_cam.argtypes = [vp, cam, vp, vp, i32, vp]
    if hasattr(L, "fid_calibrate_charuco"):  # (calibration from ChArUco corners; FID_LIB may name a build from before it)
        L.fid_calibrate_charuco.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.POINTER(FidCalibOpts), C.POINTER(FidCamera), vp, vp]
    if hasattr(L, "fid_diamonds_last"):  # (ChArUco diamonds; FID_LIB may name a build from before them)
        L.fid_default_diamond_opts.argtypes = [C.POINTER(FidDiamondOpts)]
        L.fid_default_diamond_opts.restype = None
        L.fid_diamonds_last.argtypes = [vp, C.POINTER(FidDiamondOpts), vp, i32, vp]
        L.fid_diamonds_detect.argtypes = [vp, C.POINTER(FidDiamondOpts), vp, i32, vp, i32, i32, i32, vp, i32, C.POINTER(i32)]
        L.fid_diamond_pose_cam.argtypes = [vp, C.POINTER(FidCamera), vp, i32, C.c_double, vp]
    if hasattr(L, "fid_set_rig"):  # (the camera rig; FID_LIB may name a build from before it)
        L.fid_rig_camera_from_tf.argtypes = [vp, vp, C.POINTER(FidCamera), C.POINTER(FidRigCamera)]
        L.fid_set_rig.argtypes = [vp, vp, i32]
        L.fid_rig_steps_last.argtypes = [vp, C.POINTER(i32)]
        L.fid_rig_pose_last.argtypes = [vp, vp, i32, C.c_double, vp]
        L.fid_rig_pose.argtypes = [vp, vp, vp, vp, C.c_double, vp]
    L.fid_jpeg_probe.argtypes = [vp, i64, C.POINTER(FidJpegInfo)]
    L.fid_jpeg_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.fid_jpeg_destroy.argtypes = [vp]
    L.fid_jpeg_destroy.restype = None
    L.fid_jpeg_decode.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), i32, C.c_int, vp, i64]
    L.fid_jpeg_device_ptr.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.fid_jpeg_device_ptr.restype = vp
    L.fid_jpeg_tap_bytes.argtypes = [vp, C.c_int, i32]
    L.fid_jpeg_tap_bytes.restype = i64
    L.fid_jpeg_tap_read.argtypes = [vp, C.c_int, i32, vp, i64]
    L.fid_jpeg_last_rounds.argtypes = [vp]
    L.fid_jpeg_last_rounds.restype = i32
    L.fid_jpeg_last_error.argtypes = [vp]
    L.fid_jpeg_last_error.restype = C.c_char_p
    L.fid_png_probe.argtypes = [vp, i64, C.POINTER(FidPngInfo)]
    L.fid_png_decode.argtypes = [vp, i64, C.c_int, vp, i64, C.POINTER(FidPngInfo)]
    L.fid_to_bgr.argtypes = [vp, i32, i32, i32, C.c_int, vp, i64]
    L.fid_image_to_bgr8.argtypes = [vp, i32, i32, i32, C.c_char_p, i32, vp, i64]
    if hasattr(L, "fid_encoding_from_string"):  # (ABI 7; tools/gpu_stag_ab_libs.py also loads the builds of earlier rounds through FID_LIB)
        L.fid_encoding_from_string.argtypes = [C.c_char_p, i32, C.POINTER(C.c_int), C.POINTER(i32)]
    L.fid_draw_detected_markers.argtypes = [vp, i32, i32, i32, C.POINTER(FidMarker), i32, C.c_uint32]
    if hasattr(L, "fid_to_bgr_device"):  # (the overlay on the device; FID_LIB may name a build from before it)
        L.fid_to_bgr_device.argtypes = [vp, i32, i32, i32, i32, i64, C.c_int, vp, i32, i64]
        L.fid_draw_detected_markers_device.argtypes = [vp, i32, i32, i32, i32, i64, C.POINTER(FidMarker), i32, C.POINTER(i32), C.c_uint32]
        L.fid_jpeg_marker_image.argtypes = [vp, i32, C.c_int, C.POINTER(FidMarker), i32, C.c_uint32, vp, i64]
    if hasattr(L, "fid_jpeg_enc_create"):  # (JPEG encoding on the device; FID_LIB may name a build from before it)
        L.fid_jpeg_enc_create.argtypes = [i32, i32, i32, i32, i64, C.POINTER(vp)]
        L.fid_jpeg_enc_destroy.argtypes = [vp]
        L.fid_jpeg_enc_destroy.restype = None
        L.fid_jpeg_enc_last_error.argtypes = [vp]
        L.fid_jpeg_enc_last_error.restype = C.c_char_p
        L.fid_jpeg_enc_last_ms.argtypes = [vp]
        L.fid_jpeg_enc_last_ms.restype = C.c_float
        L.fid_jpeg_enc_set.argtypes = [vp, i32, i32]
        L.fid_jpeg_encode_device.argtypes = [vp, vp, i32, i32, i32, i32, i64, C.c_int, vp, i64, C.POINTER(i64)]
        L.fid_jpeg_encode.argtypes = [vp, vp, i32, i32, i32, i32, i64, C.c_int, vp, i64, C.POINTER(i64)]
        L.fid_jpeg_enc_header.argtypes = [i32, i32, i32, i32, i32, vp, i64, C.POINTER(i64)]
        L.fid_jpeg_marker_jpeg.argtypes = [vp, i32, C.c_int, C.POINTER(FidMarker), i32, C.c_uint32, vp, vp, i64, C.POINTER(i64)]
        L.fid_jpeg_enc_tap_bytes.argtypes = [vp, i32]
        L.fid_jpeg_enc_tap_bytes.restype = i64
        L.fid_jpeg_enc_tap_read.argtypes = [vp, i32, vp, i64]
    L.fid_dict_load_file.argtypes = [C.c_char_p, i32, vp, i64, C.POINTER(FidDict)]
    L.fid_dict_last_error.argtypes = []
    L.fid_dict_last_error.restype = C.c_char_p
    L.fid_png_last_error.argtypes = []
    L.fid_png_last_error.restype = C.c_char_p
    _LIB = L
    return L
