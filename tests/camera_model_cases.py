"""Cases for the camera models of the pose kernels (fid_camera: plumb-bob, rational with thin prism, equidistant fisheye): a float64
NumPy statement of the three projections written on plain arithmetic -- no abs, no branch on a value that carries the derivative --
so that it runs on complex numbers too (the complex-step derivative is what the device's analytic Jacobian is held to), coefficient
sets, and pose_cases' generator restated for any model.  No test functions and no GPU: test_gpu_camera_models.py runs them.

The tolerance of the pose test is not chosen.  Its yardstick is the ORACLE's own deviation from the generating pose on the same
restricted geometry (sides >= 25 px, tilts 20 / 45 / 65 degrees, noise-free corners rounded to float32) over the 1 152 plumb-bob
cases of pose_cases.PAIRS, computed on the CPU: at most 2.2e-6 in |dt| / |t| and 1.0e-5 rad, apart from the wide x mild corner cases
that pose_cases.well_posed already drops.  The deviation is float32 rounding of the corners; it grows with how strongly a
distortion set bends the frame edge, which differs between sets, hence the factor 5."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import pose_cases as pc

PLUMB_BOB, RATIONAL, EQUIDISTANT = 0, 1, 2

# name: (model, coefficients)
SETS = {
    "kinect": (RATIONAL, (0.4319, -2.7146, 0.00052, -0.00031, 1.6045, 0.3122, -2.5286, 1.5265)),
    "prism12": (RATIONAL, (0.12, -0.05, 0.0008, -0.0011, 0.01, 0.03, -0.02, 0.004, 0.0009, -0.0004, -0.0007, 0.0003)),
    "fe_mild": (EQUIDISTANT, (-0.012, 0.004, -0.002, 0.0003)),
    "fe_kb": (EQUIDISTANT, (0.0759, -0.0272, 0.0118, -0.0035)),
}
# the plumb-bob set of the projection test (pose_cases' "barrel": every term present)
PROJECTION_SETS = {PLUMB_BOB: pc.DISTORTIONS["barrel"], RATIONAL: SETS["prism12"][1], EQUIDISTANT: SETS["fe_kb"][1]}

SIDES = (25.0, 80.0, 300.0)
TILTS = (20.0, 45.0, 65.0)
SIGMAS = (0.0, 0.05)
MAX_DROPPED = 0.05  # share of a camera x set's cases that the keep rule may drop

# the oracle's own deviation from the generating pose (module docstring), and what the device may deviate: five times that
ORACLE_DT_REL, ORACLE_DANGLE = 2.2e-6, 1.0e-5
TOL_DT_REL, TOL_DANGLE = 5.0 * ORACLE_DT_REL, 5.0 * ORACLE_DANGLE
# measured on the device (MI355X) over the kept noise-free cases, the largest of the 16 camera x set pairs: |dt| / |t| 2.83e-6
# (tele x fe_mild), angle 3.45e-5 rad (hd x fe_mild; every other pair stays below 1e-5); image_error - 4 sigma^2 at most 9.3e-10 px^2
DEVICE_MEASURED = "|dt|/|t| <= 2.83e-6, angle <= 3.45e-5 rad, image_error - 4 sigma^2 <= 9.3e-10 px^2"


def model_name(model: int) -> str:
    return {PLUMB_BOB: "plumb_bob", RATIONAL: "rational_polynomial", EQUIDISTANT: "equidistant"}[model]


# ---------------------------------------------------------------------------------------------- the three projections
def rodrigues(r):
    """Rotation vector -> matrix on plain arithmetic (real or complex entries; |r| > 0)."""
    r = np.asarray(r)
    th = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    k = r / th
    kx = np.array([[0.0 * th, -k[2], k[1]], [k[2], 0.0 * th, -k[0]], [-k[1], k[0], 0.0 * th]])
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


def distort(model: int, D, x, y):
    """Normalised pinhole point(s) -> distorted normalised point(s)."""
    k = list(D) + [0.0] * (12 - len(D))
    if model == EQUIDISTANT:
        r = np.sqrt(x * x + y * y)
        th = np.arctan(r)
        th2 = th * th
        thd = th * (1.0 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3]))))
        small = np.real(r) <= 1e-8
        scale = np.where(small, 1.0, thd / np.where(small, 1.0, r))
        return x * scale, y * scale
    r2 = x * x + y * y
    cd = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
    if model == RATIONAL:
        cd = cd / (1.0 + r2 * (k[5] + r2 * (k[6] + r2 * k[7])))
    xd = x * cd + 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x)
    yd = y * cd + k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y
    if model == RATIONAL:
        xd = xd + r2 * (k[8] + r2 * k[9])
        yd = yd + r2 * (k[10] + r2 * k[11])
    return xd, yd


def project(model: int, K, D, rvec_or_R, t, pts):
    """Object points (n, 3) -> pixels (n, 2) under the model; rvec_or_R a rotation vector (real or complex) or a 3 x 3 matrix."""
    R = np.asarray(rvec_or_R)
    if R.shape != (3, 3):
        R = rodrigues(R)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    pcam = np.asarray(pts, dtype=np.float64).reshape(-1, 3) @ R.T + np.asarray(t).reshape(3)
    xd, yd = distort(model, D, pcam[:, 0] / pcam[:, 2], pcam[:, 1] / pcam[:, 2])
    return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], axis=1)


def complex_step_jacobian(model: int, K, D, rvec, tvec, pts, h: float = 1e-30) -> np.ndarray:
    """d(u, v) / d(rvec, tvec) as (n, 2, 6): Im f(x + i h) / h, exact to rounding for an analytic f."""
    p0 = np.concatenate([np.asarray(rvec, dtype=np.float64), np.asarray(tvec, dtype=np.float64)])
    J = np.zeros((len(pts), 2, 6))
    for j in range(6):
        p = p0.astype(np.complex128)
        p[j] += 1j * h
        J[:, :, j] = np.imag(project(model, K, D, p[:3], p[3:], pts)) / h
    return J


def undistort_exact(model: int, D, xd: float, yd: float):
    """The normalised pinhole point whose distorted image is (xd, yd): the generator's own inverse (Newton on theta for the fisheye
    model, the fixed point run until it stands still for the others); used only to place a marker's centre in the frame."""
    if model == EQUIDISTANT:
        thd = float(np.hypot(xd, yd))
        th = thd
        for _ in range(100):
            th2 = th * th
            f = th * (1.0 + th2 * (D[0] + th2 * (D[1] + th2 * (D[2] + th2 * D[3])))) - thd
            df = 1.0 + th2 * (3 * D[0] + th2 * (5 * D[1] + th2 * (7 * D[2] + th2 * 9 * D[3])))
            th -= f / df
            if abs(f / df) < 1e-16:
                break
        s = np.tan(th) / thd if thd > 1e-12 else 1.0
        return xd * s, yd * s
    x, y = xd, yd
    for _ in range(500):
        fx, fy = distort(model, D, np.float64(x), np.float64(y))
        sx, sy = xd - float(fx), yd - float(fy)
        x, y = x + sx, y + sy
        if max(abs(sx), abs(sy)) < 1e-15:
            break
    return x, y


# ---------------------------------------------------------------------------------------------- the pose cases
@dataclass(frozen=True)
class ModelCase:
    cam: str
    set_name: str
    length: float
    side: float
    tilt: float
    sigma: float
    R: np.ndarray         # generating rotation
    tvec: np.ndarray      # generating translation
    corners: np.ndarray   # (4, 2) float32: projected by `project` under the set's model, noise added, rounded to float32
    corners0: np.ndarray  # the zero-distortion twin: the same camera, pose and noise draw with D = 0


@functools.lru_cache(maxsize=None)
def cases_for(cam: str, set_name: str) -> tuple:
    """pose_cases.cases_for's generator for one camera x coefficient set, restricted to SIDES, TILTS and SIGMAS.  The equidistant
    sets on the wide camera keep the marker centres in the middle half of the frame."""
    fx, fy, cx, cy, W, H = pc.CAMERAS[cam]
    model, D = SETS[set_name]
    K = pc.camera_matrix(cam)
    lo, hi = (0.25, 0.75) if (model == EQUIDISTANT and cam == "wide") else (0.1, 0.9)
    rng = np.random.default_rng([20241018, list(pc.CAMERAS).index(cam), list(SETS).index(set_name)])
    face = np.diag([1.0, -1.0, -1.0])
    out = []
    for length in pc.LENGTHS:
        obj = pc.square_object_points(length)
        for side in SIDES:
            z = 0.5 * (fx + fy) * length / side
            for tilt in TILTS:
                for sigma in SIGMAS:
                    for _ in range(pc.DRAWS):
                        u, v = rng.uniform(lo * W, hi * W), rng.uniform(lo * H, hi * H)
                        axis_dir, roll = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-np.pi, np.pi)
                        noise = rng.standard_normal((4, 2))
                        if z > pc.Z_MAX:
                            continue
                        nx, ny = undistort_exact(model, D, (u - cx) / fx, (v - cy) / fy)
                        R = pc.rodrigues(np.array([np.cos(axis_dir), np.sin(axis_dir), 0.0]) * np.deg2rad(tilt)) @ pc.rodrigues([0.0, 0.0, roll]) @ face
                        t = np.array([nx * z, ny * z, z])
                        c = (project(model, K, D, R, t, obj) + sigma * noise).astype(np.float32)
                        c0 = (pc.project(K, np.zeros(5), R, t, obj) + sigma * noise).astype(np.float32)
                        out.append(ModelCase(cam, set_name, length, side, tilt, sigma, R, t, c, c0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def kept(cam: str, set_name: str) -> tuple:
    """Indices of the cases whose zero-distortion twin is well-posed for the oracle (pose_cases.well_posed under
    oracle.solve_pnp_square): reads the case and the oracle only, never the library."""
    import oracle

    K = pc.camera_matrix(cam)
    keep = []
    for i, c in enumerate(cases_for(cam, set_name)):
        if pc.well_posed(c, oracle.solve_pnp_square(K, np.zeros(5), c.corners0, c.length)):
            keep.append(i)
    return tuple(keep)


def projection_points(model: int, cam: str):
    """The projection test's input: a well-posed pose and 64 object points on marker-sized squares in front of the camera (for the
    equidistant model every point within 60 degrees of the axis).  -> (rvec, tvec, points (64, 3))."""
    fx, fy, cx, cy, W, H = pc.CAMERAS[cam]
    rng = np.random.default_rng([77, model, list(pc.CAMERAS).index(cam)])
    K, D = pc.camera_matrix(cam), PROJECTION_SETS[model]
    rvec = rng.uniform(-0.6, 0.6, 3) + np.array([np.pi * 0.9, 0.0, 0.0])
    R = pc.rodrigues(rvec)
    z0 = 1.2
    span = 0.35 * z0 * min(W / fx, H / fy)  # the squares' centres: inside the middle of the frame at depth z0
    tvec = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), z0])
    pts = []
    for _ in range(16):
        c = np.array([rng.uniform(-span, span), rng.uniform(-span, span), rng.uniform(-0.1, 0.1)])
        pts.append(pc.square_object_points(rng.uniform(0.02, 0.2)) + c)
    pts = np.concatenate(pts)
    pcam = pts @ R.T + tvec
    assert (pcam[:, 2] > 0.3).all()
    if model == EQUIDISTANT:
        assert np.degrees(np.arctan(np.hypot(pcam[:, 0], pcam[:, 1]) / pcam[:, 2])).max() < 60.0
    return rvec, tvec, pts
