"""fid_camera_from_info (include/fid_abi.h), through fiducials_amd.camera.from_info: every row of the table that maps a
sensor_msgs/CameraInfo distortion_model string and coefficient count to a camera model, and what is refused with which message.
Host code: no device."""
import numpy as np
import pytest

from fiducials_amd import _lib, camera
from fiducials_amd._lib import FID_E_INVALID_ARG, FID_E_UNSUPPORTED, FidError

K = np.array([[520.0, 0.0, 325.5], [0.0, 515.0, 236.2], [0.0, 0.0, 1.0]])
D14 = np.array([0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004, 0.0009, -0.0004, -0.0007, 0.0003, 0.0, 0.0])


@pytest.mark.parametrize("name,n_D,model,n_dist", [
    ("plumb_bob", 5, camera.CAM_PLUMB_BOB, 5), ("plumb_bob", 4, camera.CAM_PLUMB_BOB, 4), ("", 5, camera.CAM_PLUMB_BOB, 5),
    ("", 4, camera.CAM_PLUMB_BOB, 4), ("rational_polynomial", 8, camera.CAM_RATIONAL, 8), ("rational_polynomial", 12, camera.CAM_RATIONAL, 12),
    ("rational_polynomial", 14, camera.CAM_RATIONAL, 12), ("equidistant", 4, camera.CAM_EQUIDISTANT, 4), ("fisheye", 4, camera.CAM_EQUIDISTANT, 4)])
def test_accepted_rows(name, n_D, model, n_dist):
    """The model, the count kept, K as given, the coefficients in order and zeros behind them (k3 = 0 for four plumb-bob ones)."""
    cam = camera.from_info(name, K, D14[:n_D])
    assert (cam.model, cam.n_dist) == (model, n_dist)
    assert np.array_equal(cam.K, K)
    assert np.array_equal(cam.D, D14[:n_dist])
    assert list(cam.c.D[n_dist:]) == [0.0] * (12 - n_dist)
    assert _lib.load().fid_camera_last_error() == b""


def test_the_struct_is_the_header_s():
    """int32 model, int32 n_dist, double K[9], double D[12]: 176 bytes, no padding."""
    import ctypes as C

    assert C.sizeof(_lib.FidCamera) == 8 + 8 * 9 + 8 * 12
    assert _lib.FidCamera.K.offset == 8 and _lib.FidCamera.D.offset == 80


def test_a_tilted_sensor_is_refused():
    D = D14.copy()
    D[13] = 0.02
    with pytest.raises(FidError) as e:
        camera.from_info("rational_polynomial", K, D)
    assert e.value.status == FID_E_UNSUPPORTED
    assert "rational_polynomial" in str(e.value) and "14" in str(e.value) and "tilt" in str(e.value)


@pytest.mark.parametrize("name,n_D", [("plumb_bob", 3), ("plumb_bob", 8), ("", 0), ("rational_polynomial", 5), ("rational_polynomial", 13),
                                      ("equidistant", 5), ("fisheye", 8), ("omnidirectional", 4), ("double_sphere", 6), ("Plumb_Bob", 5)])
def test_other_strings_and_counts_are_refused_by_name(name, n_D):
    with pytest.raises(FidError) as e:
        camera.from_info(name, K, np.zeros(n_D))
    assert e.value.status == FID_E_UNSUPPORTED
    assert f'"{name}"' in str(e.value) and f"{n_D} coefficients" in str(e.value)


def test_a_camera_that_is_no_camera_is_an_invalid_argument():
    for bad in ((0, 0), (1, 1)):  # fx, fy
        Kb = K.copy()
        Kb[bad] = 0.0
        with pytest.raises(FidError) as e:
            camera.from_info("plumb_bob", Kb, np.zeros(5))
        assert e.value.status == FID_E_INVALID_ARG
    for v in (np.nan, np.inf):
        Kb = K.copy()
        Kb[0, 2] = v
        with pytest.raises(FidError) as e:
            camera.from_info("plumb_bob", Kb, np.zeros(5))
        assert e.value.status == FID_E_INVALID_ARG
        Db = np.zeros(8)
        Db[6] = v
        with pytest.raises(FidError) as e:
            camera.from_info("rational_polynomial", K, Db)
        assert e.value.status == FID_E_INVALID_ARG


def test_camera_or_K_and_D_never_both():
    cam = camera.from_info("equidistant", K, np.zeros(4))
    assert camera.resolve(None, None, cam) is cam
    plumb = camera.resolve(K, None, None)
    assert plumb.model == camera.CAM_PLUMB_BOB and plumb.n_dist == 5 and not plumb.D.any()
    assert np.array_equal(camera.resolve(K, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], None).D, [0.1, 0.2, 0.3, 0.4, 0.5])
    assert camera.resolve(None, None, None) is None
    for args in ((K, None), (None, np.zeros(5)), (K, np.zeros(5))):
        with pytest.raises(ValueError):
            camera.resolve(args[0], args[1], cam)
