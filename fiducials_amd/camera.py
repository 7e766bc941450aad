"""The camera as a value (fid_camera, include/fid_abi.h): the intrinsics with their distortion MODEL -- plumb-bob, rational
polynomial with thin prism, or the equidistant fisheye model -- as sensor_msgs/CameraInfo names it.  Every pose method of
ArucoDetector, StagDetector and StagPool takes `camera=` in place of `K, D`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import CAM_EQUIDISTANT, CAM_PLUMB_BOB, CAM_RATIONAL, FidCamera, FidError, FidRigCamera

MODEL_NAMES = {CAM_PLUMB_BOB: "plumb_bob", CAM_RATIONAL: "rational_polynomial", CAM_EQUIDISTANT: "equidistant"}


class Camera:
    """A fid_camera.  `model` is CAM_PLUMB_BOB / CAM_RATIONAL / CAM_EQUIDISTANT, `K` the 3 x 3 matrix, `D` the coefficients given
    (n_dist of them).  Build one with from_info (the CameraInfo road, which checks the model string and the count) or directly."""

    def __init__(self, model: int, K, D=()):
        D = np.asarray(D, dtype=np.float64).reshape(-1)
        if len(D) > 12:
            raise ValueError(f"a camera carries at most 12 distortion coefficients, not {len(D)}")
        self.c = FidCamera()
        self.c.model = int(model)
        self.c.n_dist = len(D)
        self.c.K[:] = [float(v) for v in np.asarray(K, dtype=np.float64).reshape(9)]
        self.c.D[:] = [float(v) for v in D] + [0.0] * (12 - len(D))

    @classmethod
    def _from_struct(cls, c: FidCamera) -> "Camera":
        self = cls.__new__(cls)
        self.c = c
        return self

    @property
    def model(self) -> int:
        return int(self.c.model)

    @property
    def n_dist(self) -> int:
        return int(self.c.n_dist)

    @property
    def K(self) -> np.ndarray:
        return np.array(self.c.K[:], dtype=np.float64).reshape(3, 3)

    @property
    def D(self) -> np.ndarray:
        return np.array(self.c.D[:self.n_dist], dtype=np.float64)

    def to_info(self):
        """Camera -> (distortion_model, K (3, 3), D) as sensor_msgs/CameraInfo carries them (fid_camera_to_info, the inverse of
        from_info): "plumb_bob" with 5 coefficients, "rational_polynomial" with 8 or 12, "equidistant" with 4."""
        L = _lib.load()
        name = C.create_string_buffer(32)
        K = (C.c_double * 9)()
        D = (C.c_double * 12)()
        n = C.c_int32(0)
        rc = L.fid_camera_to_info(C.byref(self.c), name, K, D, C.byref(n))
        if rc != _lib.FID_OK:
            raise FidError(rc, "fid_camera_to_info: the camera's model or coefficient count is outside the ABI's")
        return name.value.decode(), np.array(K[:], dtype=np.float64).reshape(3, 3), np.array(D[:n.value], dtype=np.float64)

    def __repr__(self) -> str:
        return f"Camera({MODEL_NAMES.get(self.model, self.model)}, K={self.K.tolist()}, D={self.D.tolist()})"


def from_info(distortion_model: str, K, D) -> Camera:
    """sensor_msgs/CameraInfo -> Camera (fid_camera_from_info): "plumb_bob" or "" with 4 or 5 coefficients, "rational_polynomial"
    with 8, 12, or 14 whose tilt terms are zero, "equidistant" / "fisheye" with 4.  Anything else raises FidError
    (FID_E_UNSUPPORTED) with a message that names what was given; a K with zero fx or fy, or a value that is not finite, raises
    FidError (FID_E_INVALID_ARG).  Host code: no device is touched."""
    L = _lib.load()
    Kc = (C.c_double * 9)(*np.asarray(K, dtype=np.float64).reshape(9))
    Dv = np.asarray(D, dtype=np.float64).reshape(-1)
    Dc = (C.c_double * max(len(Dv), 1))(*Dv)
    out = FidCamera()
    rc = L.fid_camera_from_info(str(distortion_model).encode(), Kc, Dc, len(Dv), C.byref(out))
    if rc != _lib.FID_OK:
        raise FidError(rc, L.fid_camera_last_error().decode())
    return Camera._from_struct(out)


class RigCamera:
    """A fid_rig_camera: a camera of a rig with the RIG frame in the CAMERA frame, X_cam = R X_rig + t (solvePnP's convention).
    from_tf takes what a static transform says instead: the camera's pose in the rig frame."""

    def __init__(self, camera: Camera, R, t):
        if not isinstance(camera, Camera):
            raise TypeError("RigCamera takes a fiducials_amd.camera.Camera")
        self.c = FidRigCamera()
        C.memmove(C.byref(self.c.cam), C.byref(camera.c), C.sizeof(FidCamera))
        self.c.R[:] = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)]
        self.c.t[:] = [float(v) for v in np.asarray(t, dtype=np.float64).reshape(3)]

    @classmethod
    def from_tf(cls, xyz, quat, camera: Camera) -> "RigCamera":
        """The camera at position xyz with orientation quat (x, y, z, w) in the rig frame -- a base_link -> camera_optical_frame
        transform -- inverted (fid_rig_camera_from_tf).  Host code: no device is touched."""
        L = _lib.load()
        p = (C.c_double * 3)(*np.asarray(xyz, dtype=np.float64).reshape(3))
        q = (C.c_double * 4)(*np.asarray(quat, dtype=np.float64).reshape(4))
        self = cls.__new__(cls)
        self.c = FidRigCamera()
        rc = L.fid_rig_camera_from_tf(p, q, C.byref(camera.c), C.byref(self.c))
        if rc != _lib.FID_OK:
            raise FidError(rc, "fid_rig_camera_from_tf: xyz and quat must be finite and the quaternion not zero")
        return self

    @property
    def camera(self) -> Camera:
        c = FidCamera()
        C.memmove(C.byref(c), C.byref(self.c.cam), C.sizeof(FidCamera))
        return Camera._from_struct(c)

    @property
    def R(self) -> np.ndarray:
        return np.array(self.c.R[:], dtype=np.float64).reshape(3, 3)

    @property
    def t(self) -> np.ndarray:
        return np.array(self.c.t[:], dtype=np.float64)

    def __repr__(self) -> str:
        return f"RigCamera({self.camera!r}, R={self.R.tolist()}, t={self.t.tolist()})"


def resolve(K, D, camera: Camera | None) -> Camera | None:
    """What a pose method was handed: `camera=`, or K and D (the plumb-bob camera, D's first five), never both.  None when there
    is neither (the callers that allow that skip the pose step)."""
    if camera is not None:
        if K is not None or D is not None:
            raise ValueError("pass either camera= or K, D -- not both")
        if not isinstance(camera, Camera):
            raise TypeError("camera= takes a fiducials_amd.camera.Camera")
        return camera
    if K is None:
        return None
    Dv = np.zeros(5) if D is None else np.asarray(D, dtype=np.float64).reshape(-1)[:5]
    Dv = np.concatenate([Dv, np.zeros(5 - len(Dv))])
    return Camera(CAM_PLUMB_BOB, K, Dv)
