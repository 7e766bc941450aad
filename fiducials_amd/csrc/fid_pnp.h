// fid_pnp.h -- cv::solvePnP (SOLVEPNP_ITERATIVE) as a device library: what k_pose (fid_kernels.hip K8), k_stag_pose and
// k_stag_bundle_pose (fid_stag_pose.hip K17, K18), k_map_pose (fid_map_pose.hip K19), k_map_pose_robust (fid_map_pose_robust.hip
// K20) and k_charuco_pose (fid_charuco.hip) have in common.  Included once, ahead of K8, in the fid_api.hip translation unit
// (needs WAVE and <float.h> from fid_kernels.hip's head).
//
//   lane-group sums      shfl_xor_f64, dpp_f64, grp_sum8, grp_sum16, wave_sum_f64
//   the camera           PoseCam, pose_cam_from (fid_camera -> PoseCam), POSE_CAM_DISPATCH (the host picks the instantiation)
//   rotations            jacobi3, rodrigues_m2v, rodrigues_v2m (cvRodrigues2 with dR/dr), pnp_mul3
//   projection           project_one<MODEL> (cvProjectPoints2 for one residual with its analytic Jacobian row: plumb-bob, rational
//                        with thin prism, or the cv::fisheye equidistant model)
//   cvUndistortPoints    pnp_undistort<MODEL> (false: the equidistant model has no pinhole point for this pixel)
//   the start            pnp_quad_homography, pnp_pose_from_h (four corners, closed form); pnp_scatter_eig, pnp_plane_frame,
//                        pnp_dlt_entry, pnp_smallest_eigvec9, pnp_dlt_finish (coplanar sets: findHomography's DLT);
//                        pnp_start_largest (sets that are not coplanar)
//   CvLevMarq            lm_lambda, solve6_spd, LevMarq
//   the covariance       pnp_covariance, pnp_cov_zero (sigma^2 (J^T J)^-1 at the returned pose, in the ROS pose convention)
//   the wave-strided     pnp_wave_solve over a view of a kernel's points (planarity, either start, CvLevMarq, the reprojection
//   solve                error), with pnp_homography_dlt and pnp_wave_residuals (also the covariance's J^T J); the record's
//                        pose part: pnp_pose_record, pnp_pose_record_zero
//
// A kernel gathers its points, makes the start, and runs
//     LevMarq lm;
//     bool needJ = true;
//     do { residuals at param; with needJ: reduce S, gJ } while (lm.step(param, S, gJ, errSq, needJ));  (errSq: a callable, see LevMarq)
// with a reduction over its lanes.  The order of a floating-point sum is part of a kernel's result, so a reduction is shared only
// where the order is the same.  ONE form is: a wave per point set with strided per-lane partial sums and a butterfly, the order of
// k_map_pose, k_map_pose_robust and k_charuco_pose, which run pnp_wave_solve (at the end of this file) on their views.  The other
// three are each one kernel's own: eight lanes by DPP (k_pose), sixteen lanes (k_stag_pose), a wave with two residuals per lane
// and sequential sums (k_stag_bundle_pose).
//
// The camera model (fid_camera_model, fid_abi.h) is a TEMPLATE parameter of project_one, pnp_undistort, pnp_start_largest,
// pnp_wave_solve and of the kernels: nothing inside the Levenberg-Marquardt loop asks for it at run time.  The FID_CAM_PLUMB_BOB instantiation is the code
// as it was before the models came (the same expressions in the same order); FID_CAM_RATIONAL adds OpenCV 4.2's terms so that with
// k4..k6 and s1..s4 zero every intermediate value equals the plumb-bob one (x * 1.0, + 0.0).
#pragma once

// LDS hand-over inside ONE wave: what a lane wrote before is what every lane reads after (named after k_stag_refine, its first user)
#define SR_LDS_SYNC()                                          \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
    } while (0)

__device__ __forceinline__ double shfl_xor_f64(double v, int mask)
{
    unsigned long long u = __double_as_longlong(v);
    unsigned lo = __shfl_xor((unsigned)u, mask, WAVE);
    unsigned hi = __shfl_xor((unsigned)(u >> 32), mask, WAVE);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
// a double from the lane a DPP control names (two v_mov_b32 with a DPP operand: no trip through the LDS crossbar)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    const unsigned long long u = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
// sum over an aligned group of eight lanes, in every lane of the group.  The same three additions with the same operands as the
// xor-shuffle form (lane ^ 1: quad_perm [1,0,3,2]; lane ^ 2: quad_perm [2,3,0,1]; the other quad of the group: row_half_mirror
// -- after the second step every lane of a quad holds the same value, so lane 7 - i serves as well as lane i ^ 4), without the
// six ds_bpermute round trips: Levenberg-Marquardt reduces 28 such sums per iteration, 84 dependent LDS latencies that were
// most of k_pose's time.
__device__ __forceinline__ double grp_sum8(double v)
{
    v += dpp_f64<0xB1>(v);
    v += dpp_f64<0x4E>(v);
    v += dpp_f64<0x141>(v);
    return v;
}
__device__ __forceinline__ double grp_sum16(double v)
{
    v += shfl_xor_f64(v, 1);
    v += shfl_xor_f64(v, 2);
    v += shfl_xor_f64(v, 4);
    v += shfl_xor_f64(v, 8);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v)
{
    v += shfl_xor_f64(v, 1);
    v += shfl_xor_f64(v, 2);
    v += shfl_xor_f64(v, 4);
    v += shfl_xor_f64(v, 8);
    v += shfl_xor_f64(v, 16);
    v += shfl_xor_f64(v, 32);
    return v;
}

struct PoseCam {
    double K[9];
    double D[12];  // plumb-bob: k1 k2 p1 p2 k3; rational: + k4 k5 k6 s1 s2 s3 s4; equidistant: k1..k4 -- zero beyond what the model has
    double fiducial_len;
    int model;  // fid_camera_model: which instantiation the host launched (the kernels do not read it)
    template <class V>
    __host__ __device__ __forceinline__ void visit(V &&v)
    {
        v(K); v(D); v(fiducial_len); v(model);
    }
};
// the caller's camera as the kernels take it; D beyond n_dist is zero whatever the caller left there
static inline PoseCam pose_cam_from(const fid_camera &c, double fiducial_len)
{
    PoseCam p;
    for (int i = 0; i < 9; i++) p.K[i] = c.K[i];
    for (int i = 0; i < 12; i++) p.D[i] = i < c.n_dist ? c.D[i] : 0.;
    p.fiducial_len = fiducial_len;
    p.model = c.model;
    return p;
}
// {FID_CAM_PLUMB_BOB, 5, K, D}: what the entry points without a fid_camera hand to their _cam twins (D == NULL: no distortion)
static inline fid_camera fid_camera_plumb_bob(const double K[9], const double D[5])
{
    fid_camera c;
    c.model = FID_CAM_PLUMB_BOB;
    c.n_dist = 5;
    for (int i = 0; i < 9; i++) c.K[i] = K[i];
    for (int i = 0; i < 12; i++) c.D[i] = (D && i < 5) ? D[i] : 0.;
    return c;
}
// a fid_camera as it is remembered and compared: D beyond n_dist zeroed
static inline fid_camera fid_camera_normalised(const fid_camera &in)
{
    fid_camera c = in;
    for (int i = 0; i < 12; i++)
        if (i >= c.n_dist) c.D[i] = 0.;
    return c;
}
static inline bool fid_camera_usable(const fid_camera *c)
{
    return c && c->model >= FID_CAM_PLUMB_BOB && c->model <= FID_CAM_EQUIDISTANT && c->n_dist >= 0 && c->n_dist <= 12;
}
// sigma_px of a _cov entry point: zero (the a-posteriori estimate) or positive, and finite
static inline bool fid_sigma_usable(double sigma_px) { return sigma_px >= 0. && sigma_px - sigma_px == 0.; }
// the host's choice of instantiation: STMT is expanded once per model with the constant CAM_MODEL in scope
#define POSE_CAM_DISPATCH(model, STMT)                         \
    do {                                                       \
        switch (model) {                                       \
        case FID_CAM_RATIONAL: {                               \
            constexpr int CAM_MODEL = FID_CAM_RATIONAL;        \
            STMT;                                              \
        } break;                                               \
        case FID_CAM_EQUIDISTANT: {                            \
            constexpr int CAM_MODEL = FID_CAM_EQUIDISTANT;     \
            STMT;                                              \
        } break;                                               \
        default: {                                             \
            constexpr int CAM_MODEL = FID_CAM_PLUMB_BOB;       \
            STMT;                                              \
        } break;                                               \
        }                                                      \
    } while (0)
// the equidistant model's pinhole normalisation ends at 90 degrees off the axis; a corner at or beyond this angle cannot be posed
#define PNP_FISHEYE_MAX_THETA (89. * 3.14159265358979323846 / 180.)
// CvLevMarq's damping factor exp(lambdaLg10 * log(10.)) for lambdaLg10 = -16 .. 16 as the HOST's libm gives it (glibc's exp / log,
// what the reference runs on; generated with Python's math.exp(k * math.log(10.0)), hexadecimal literals = the exact doubles):
// a table look-up instead of a device exp() in every Levenberg-Marquardt step -- and the reference's values, not the device
// library's.
__device__ __forceinline__ double lm_lambda(int lg10)
{
    static const double t[33] = {0x1.cd2b297d889a0p-54, 0x1.203af9ee755f8p-50, 0x1.6849b86a12b93p-47, 0x1.c25c268497664p-44, 0x1.19799812dea04p-40, 0x1.5fd7fe179648cp-37, 0x1.b7cdfd9d7bd9cp-34, 0x1.12e0be826d687p-30, 0x1.5798ee2308c2fp-27, 0x1.ad7f29abcaf44p-24, 0x1.0c6f7a0b5ed87p-20, 0x1.4f8b588e368e5p-17, 0x1.a36e2eb1c4326p-14, 0x1.0624dd2f1a9f9p-10, 0x1.47ae147ae1478p-7, 0x1.9999999999998p-4, 0x1.0000000000000p+0, 0x1.4000000000001p+3, 0x1.9000000000003p+6, 0x1.f400000000006p+9, 0x1.3880000000005p+13, 0x1.86a000000000ep+16, 0x1.e84800000000bp+19, 0x1.312d000000003p+23, 0x1.7d7840000000cp+26, 0x1.dcd6500000018p+29, 0x1.2a05f20000015p+33, 0x1.74876e800000ap+36, 0x1.d1a94a2000015p+39, 0x1.2309ce5400013p+43, 0x1.6bcc41e900008p+46, 0x1.c6bf52634002fp+49, 0x1.1c37937e08011p+53};
    lg10 = lg10 < -16 ? -16 : (lg10 > 16 ? 16 : lg10);
    return t[lg10 + 16];
}

// symmetric 3x3 eigen-decomposition by cyclic Jacobi, fully unrolled (static register indexing)
__device__ __forceinline__ void jacobi3(double A[3][3], double V[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1. : 0.;
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        double dg = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off <= 1e-60 * dg || off < 1e-300) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                double apq = A[p][q];
                if (fabs(apq) < 1e-300) continue;
                double theta = (A[q][q] - A[p][p]) / (2. * apq);
                double t = (theta >= 0 ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                double c = 1. / sqrt(t * t + 1.), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double vpk = V[p][k], vqk = V[q][k];
                    V[p][k] = c * vpk - s * vqk;
                    V[q][k] = s * vpk + c * vqk;
                }
            }
    }
}

// R <- U * Vt of its SVD  ( = R * (RtR)^(-1/2) ), as cvRodrigues2 does before reading the axis
__device__ __forceinline__ void orthonormalize3(double R[9])
{
    double A[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) A[i][j] = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j];
    jacobi3(A, V);
    double Pm[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Pm[i][j] = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double w = A[k][k];
        double is = w > 1e-300 ? 1. / sqrt(w) : 0.;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Pm[i][j] += V[k][i] * V[k][j] * is;
    }
    double T[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) T[i * 3 + j] = R[i * 3] * Pm[0][j] + R[i * 3 + 1] * Pm[1][j] + R[i * 3 + 2] * Pm[2][j];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = T[i];
}

__device__ __forceinline__ void rodrigues_m2v(const double Rin[9], double r[3])
{
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = Rin[i];
    orthonormalize3(R);
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = acos(c);
    if (s < 1e-5) {
        double t;
        if (c > 0)
            rx = ry = rz = 0;
        else {
            t = (R[0] + 1) * 0.5;
            rx = sqrt(t > 0. ? t : 0.);
            t = (R[4] + 1) * 0.5;
            ry = sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
            t = (R[8] + 1) * 0.5;
            rz = sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
            if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
            theta /= sqrt(rx * rx + ry * ry + rz * rz);
            rx *= theta;
            ry *= theta;
            rz *= theta;
        }
    } else {
        double vth = 1 / (2 * s);
        vth *= theta;
        rx *= vth;
        ry *= vth;
        rz *= vth;
    }
    r[0] = rx;
    r[1] = ry;
    r[2] = rz;
}

// cvRodrigues2 vector -> matrix with dR/dr (J[i*9+k] = dR_k / dr_i)
__device__ __forceinline__ void rodrigues_v2m(const double r_in[3], double R[9], double J[27], bool wantJ)
{
    double rx = r_in[0], ry = r_in[1], rz = r_in[2];
    double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1. : 0.;
        if (wantJ) {
#pragma unroll
            for (int i = 0; i < 27; i++) J[i] = 0;
            J[5] = J[15] = J[19] = -1;
            J[7] = J[11] = J[21] = 1;
        }
        return;
    }
    double c, s;
    sincos(theta, &s, &c);  // (one argument reduction for the pair)
    const double c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = c * ((k % 4 == 0) ? 1. : 0.) + c1 * rrt[k] + s * r_x[k];
    if (wantJ) {
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double drrt[27] = {rx + rx, ry, rz, ry, 0,       0,  rz, 0,  0,       0, rx, 0, rx, ry + ry,
                                 rz,      0,  rz, 0,  0,       0,  rx, 0,  0,       ry, rx, ry, rz + rz};
        const double d_r_x_[27] = {0, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double ri = i == 0 ? rx : i == 1 ? ry : rz;
            double a0 = -s * ri, a1 = (s - 2 * c1 * itheta) * ri, a2 = c1 * itheta;
            double a3 = (c - s * itheta) * ri, a4 = s * itheta;
#pragma unroll
            for (int k = 0; k < 9; k++)
                J[i * 9 + k] = a0 * I[k] + a1 * rrt[k] + a2 * drrt[i * 9 + k] + a3 * r_x[k] + a4 * d_r_x_[i * 9 + k];
        }
    }
}

// cvProjectPoints2Internal for ONE object point and ONE image coordinate (sel = 0: x, 1: y);
// Jrow[0..2] = d/d rvec, Jrow[3..5] = d/d tvec.  k: PoseCam::D.
//   FID_CAM_PLUMB_BOB    k1 k2 p1 p2 k3
//   FID_CAM_RATIONAL     + the denominator 1 + k4 r2 + k5 r4 + k6 r6 (icdist2) and the thin prism s1..s4, OpenCV 4.2's expressions
//   FID_CAM_EQUIDISTANT  cv::fisheye: theta = atan r, theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
//                        (u, v) = (fx a, fy b) theta_d / r + (cx, cy) (the scale is 1 where r <= 1e-8); no skew
template <int MODEL>
__device__ __forceinline__ double project_one(const double M[3], const double param[6], const double K[9], const double k[12],
                                               int sel, double Jrow[6], bool wantJ)
{
    double R[9], dRdr[27];
    rodrigues_v2m(param, R, dRdr, wantJ);
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double X = M[0], Y = M[1], Z = M[2];
    double x = R[0] * X + R[1] * Y + R[2] * Z + param[3];
    double y = R[3] * X + R[4] * Y + R[5] * Z + param[4];
    double z = R[6] * X + R[7] * Y + R[8] * Z + param[5];
    z = z ? 1. / z : 1;
    x *= z;
    y *= z;
    if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
        const double r2 = x * x + y * y, r = sqrt(r2);
        const double th = atan(r), th2 = th * th;
        const double poly = 1 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3])));
        const double thd = th * poly;
        const bool tiny = !(r > 1e-8);
        const double scale = tiny ? 1. : thd / r;
        const double out = sel == 0 ? fx * (x * scale) + cx : fy * (y * scale) + cy;
        if (wantJ) {
            // d scale = g * (x dx + y dy):  d scale / d r = (theta_d' / (1 + r2) - scale) / r,  d r = (x dx + y dy) / r
            const double dpoly = 1 + th2 * (3 * k[0] + th2 * (5 * k[1] + th2 * (7 * k[2] + th2 * (9 * k[3]))));
            const double g = tiny ? 0. : (dpoly / (1 + r2) - scale) / r2;
            const double dxdt[3] = {z, 0, -x * z}, dydt[3] = {0, z, -y * z};
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double ds = g * (x * dxdt[j] + y * dydt[j]);
                Jrow[3 + j] = sel == 0 ? fx * (dxdt[j] * scale + x * ds) : fy * (dydt[j] * scale + y * ds);
            }
            const double dx0dr[3] = {X * dRdr[0] + Y * dRdr[1] + Z * dRdr[2], X * dRdr[9] + Y * dRdr[10] + Z * dRdr[11],
                                     X * dRdr[18] + Y * dRdr[19] + Z * dRdr[20]};
            const double dy0dr[3] = {X * dRdr[3] + Y * dRdr[4] + Z * dRdr[5], X * dRdr[12] + Y * dRdr[13] + Z * dRdr[14],
                                     X * dRdr[21] + Y * dRdr[22] + Z * dRdr[23]};
            const double dz0dr[3] = {X * dRdr[6] + Y * dRdr[7] + Z * dRdr[8], X * dRdr[15] + Y * dRdr[16] + Z * dRdr[17],
                                     X * dRdr[24] + Y * dRdr[25] + Z * dRdr[26]};
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double dxdr = z * (dx0dr[j] - x * dz0dr[j]);
                const double dydr = z * (dy0dr[j] - y * dz0dr[j]);
                const double ds = g * (x * dxdr + y * dydr);
                Jrow[j] = sel == 0 ? fx * (dxdr * scale + x * ds) : fy * (dydr * scale + y * ds);
            }
        }
        return out;
    } else {
        double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
        double cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6;
        double icdist2 = 1.;
        if constexpr (MODEL == FID_CAM_RATIONAL) icdist2 = 1. / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
        double xd = x * cdist * icdist2 + k[2] * a1 + k[3] * a2;
        double yd = y * cdist * icdist2 + k[2] * a3 + k[3] * a1;
        if constexpr (MODEL == FID_CAM_RATIONAL) {
            xd = xd + k[8] * r2 + k[9] * r4;
            yd = yd + k[10] * r2 + k[11] * r4;
        }
        double out = sel == 0 ? xd * fx + cx : yd * fy + cy;
        if (wantJ) {
            const double dxdt[3] = {z, 0, -x * z}, dydt[3] = {0, z, -y * z};
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double dr2dt = 2 * x * dxdt[j] + 2 * y * dydt[j];
                double dcdist_dt = k[0] * dr2dt + 2 * k[1] * r2 * dr2dt + 3 * k[4] * r4 * dr2dt;
                double da1dt = 2 * (x * dydt[j] + y * dxdt[j]);
                double dmxdt, dmydt;
                if constexpr (MODEL == FID_CAM_RATIONAL) {
                    double dicdist2_dt = -icdist2 * icdist2 * (k[5] * dr2dt + 2 * k[6] * r2 * dr2dt + 3 * k[7] * r4 * dr2dt);
                    dmxdt = (dxdt[j] * cdist * icdist2 + x * dcdist_dt * icdist2 + x * cdist * dicdist2_dt + k[2] * da1dt + k[3] * (dr2dt + 4 * x * dxdt[j]) +
                             k[8] * dr2dt + 2 * r2 * k[9] * dr2dt);
                    dmydt = (dydt[j] * cdist * icdist2 + y * dcdist_dt * icdist2 + y * cdist * dicdist2_dt + k[2] * (dr2dt + 4 * y * dydt[j]) + k[3] * da1dt +
                             k[10] * dr2dt + 2 * r2 * k[11] * dr2dt);
                } else {
                    dmxdt = (dxdt[j] * cdist * icdist2 + x * dcdist_dt * icdist2 + k[2] * da1dt + k[3] * (dr2dt + 4 * x * dxdt[j]));
                    dmydt = (dydt[j] * cdist * icdist2 + y * dcdist_dt * icdist2 + k[2] * (dr2dt + 4 * y * dydt[j]) + k[3] * da1dt);
                }
                Jrow[3 + j] = sel == 0 ? fx * dmxdt : fy * dmydt;
            }
            const double dx0dr[3] = {X * dRdr[0] + Y * dRdr[1] + Z * dRdr[2], X * dRdr[9] + Y * dRdr[10] + Z * dRdr[11],
                                     X * dRdr[18] + Y * dRdr[19] + Z * dRdr[20]};
            const double dy0dr[3] = {X * dRdr[3] + Y * dRdr[4] + Z * dRdr[5], X * dRdr[12] + Y * dRdr[13] + Z * dRdr[14],
                                     X * dRdr[21] + Y * dRdr[22] + Z * dRdr[23]};
            const double dz0dr[3] = {X * dRdr[6] + Y * dRdr[7] + Z * dRdr[8], X * dRdr[15] + Y * dRdr[16] + Z * dRdr[17],
                                     X * dRdr[24] + Y * dRdr[25] + Z * dRdr[26]};
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double dxdr = z * (dx0dr[j] - x * dz0dr[j]);
                double dydr = z * (dy0dr[j] - y * dz0dr[j]);
                double dr2dr = 2 * x * dxdr + 2 * y * dydr;
                double dcdist_dr = (k[0] + 2 * k[1] * r2 + 3 * k[4] * r4) * dr2dr;
                double da1dr = 2 * (x * dydr + y * dxdr);
                double dmxdr, dmydr;
                if constexpr (MODEL == FID_CAM_RATIONAL) {
                    double dicdist2_dr = -icdist2 * icdist2 * (k[5] + 2 * k[6] * r2 + 3 * k[7] * r4) * dr2dr;
                    dmxdr = (dxdr * cdist * icdist2 + x * dcdist_dr * icdist2 + x * cdist * dicdist2_dr + k[2] * da1dr + k[3] * (dr2dr + 4 * x * dxdr) +
                             (k[8] + 2 * r2 * k[9]) * dr2dr);
                    dmydr = (dydr * cdist * icdist2 + y * dcdist_dr * icdist2 + y * cdist * dicdist2_dr + k[2] * (dr2dr + 4 * y * dydr) + k[3] * da1dr +
                             (k[10] + 2 * r2 * k[11]) * dr2dr);
                } else {
                    dmxdr = (dxdr * cdist * icdist2 + x * dcdist_dr * icdist2 + k[2] * da1dr + k[3] * (dr2dr + 4 * x * dxdr));
                    dmydr = (dydr * cdist * icdist2 + y * dcdist_dr * icdist2 + k[2] * (dr2dr + 4 * y * dydr) + k[3] * da1dr);
                }
                Jrow[j] = sel == 0 ? fx * dmxdr : fy * dmydr;
            }
        }
        return out;
    }
}

// solve (JtJ with its diagonal scaled by 1 + lambda) x = JtErr, JtJ symmetric positive definite (packed upper
// triangle, row-major: index of (a, b), a <= b, is a*6 - a*(a-1)/2 + (b - a)); LDL^T, unrolled
__device__ __forceinline__ void solve6_spd(const double S[21], const double g[6], double lambda, double x[6])
{
    double A[6][6];
    {
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) {
                A[a][b] = S[idx];
                A[b][a] = S[idx];
                idx++;
            }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) A[i][i] *= 1. + lambda;
    double L[6][6], Dg[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * Dg[k];
        Dg[j] = d;
        double id = d != 0. ? 1. / d : 0.;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * Dg[k];
            L[i][j] = v * id;
        }
    }
    double yv[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = g[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k] * yv[k];
        yv[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double v = Dg[i] != 0. ? yv[i] / Dg[i] : 0.;
#pragma unroll
        for (int k = i + 1; k < 6; k++) v -= L[k][i] * x[k];
        x[i] = v;
    }
}

// The covariance of a returned pose (fid_abi.h: "pose covariance").  S: the 21 packed sums of J^T J at p (solve6_spd's order), e2:
// |e|^2 at p, n_points: N, p: (rvec, tvec), sigma_px: the caller's pixel sigma (0: the a-posteriori sigma^2 = e2 / (2 N - 6)).
// (J^T J)^-1 by the LDL^T of solve6_spd without damping -- L^-1 by forward substitution, then L^-T D^-1 L^-1, one triangle --,
// times sigma^2 as the last step: cov_rt.  cov_pose = A cov_rt A^T with A = [[0, I], [J_l(rvec), 0]] and, with CAM, cov_cam_pose =
// B cov_pose B^T with B = [[-R^T, -R^T [t]x], [0, -R^T]], both in their 3 x 3 blocks (the zero blocks are not multiplied).  Every
// matrix is written as one triangle and its mirror.  Everything in registers with static indices; the record goes straight to
// memory, entry by entry, so that no 6 x 6 result is held beyond its use.  One lane calls it.
__device__ __forceinline__ void pnp_cov_zero(fid_pose_cov *o, int status, int n_points, double *cov_cam_pose)
{
    o->status = status;
    o->n_points = n_points;
    o->sigma2 = 0.;
    for (int i = 0; i < 36; i++) o->cov_rt[i] = o->cov_pose[i] = 0.;
    if (cov_cam_pose)
        for (int i = 0; i < 36; i++) cov_cam_pose[i] = 0.;
}
template <bool CAM>
__device__ __forceinline__ void pnp_covariance(const double S[21], double e2, int n_points, const double p[6], double sigma_px, fid_pose_cov *o,
                                               double *cov_cam_pose)
{
    // ---- LDL^T of J^T J (solve6_spd's factorisation, lambda = 0)
    double A[6][6];
    {
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) {
                A[a][b] = S[idx];
                A[b][a] = S[idx];
                idx++;
            }
    }
    double L[6][6], Dg[6], iD[6];
    bool good = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * Dg[k];
        good = good && d > 0. && d - d == 0.;  // (a pivot that is not positive, or not finite: status 2)
        const double id = 1. / d;
        Dg[j] = d;
        iD[j] = id;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * Dg[k];
            L[i][j] = v * id;
        }
    }
    if (!good) {
        pnp_cov_zero(o, 2, n_points, CAM ? cov_cam_pose : nullptr);
        return;
    }
    // ---- M = L^-1 (unit lower triangle), C = M^T D^-1 M
    double M[6][6];
#pragma unroll
    for (int j = 0; j < 6; j++)
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = -L[i][j];
#pragma unroll
            for (int k = j + 1; k < i; k++) v -= L[i][k] * M[k][j];
            M[i][j] = v;
        }
    const double sigma2 = sigma_px > 0. ? sigma_px * sigma_px : e2 / (double)(2 * n_points - 6);
    double C[6][6];  // cov_rt
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) {
            // sum over k >= b of M[k][a] M[k][b] / D[k], M[k][k] = 1
            double v = (a == b ? 1. : M[b][a]) * iD[b];
#pragma unroll
            for (int k = b + 1; k < 6; k++) v += M[k][a] * M[k][b] * iD[k];
            v *= sigma2;
            C[a][b] = v;
            C[b][a] = v;
        }
    o->status = 0;
    o->n_points = n_points;
    o->sigma2 = sigma2;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) o->cov_rt[6 * a + b] = C[a][b];
    // ---- J_l(rvec) = I + (1 - cos th) / th^2 [r]x + (th - sin th) / th^3 [r]x^2, [r]x^2 = r r^T - th^2 I
    double Jl[3][3];
    {
        const double rx = p[0], ry = p[1], rz = p[2];
        const double th2 = rx * rx + ry * ry + rz * rz, th = sqrt(th2);
        double ca = 0.5, cb = 1. / 6.;
        if (!(th < 1e-4)) {
            double sn, cs;
            sincos(th, &sn, &cs);
            ca = (1. - cs) / th2;
            cb = (th - sn) / (th2 * th);
        }
        Jl[0][0] = 1. + cb * (rx * rx - th2); Jl[0][1] = -ca * rz + cb * rx * ry;   Jl[0][2] = ca * ry + cb * rx * rz;
        Jl[1][0] = ca * rz + cb * rx * ry;    Jl[1][1] = 1. + cb * (ry * ry - th2); Jl[1][2] = -ca * rx + cb * ry * rz;
        Jl[2][0] = -ca * ry + cb * rx * rz;   Jl[2][1] = ca * rx + cb * ry * rz;    Jl[2][2] = 1. + cb * (rz * rz - th2);
    }
    // ---- cov_pose = [[Ctt, Ctr Jl^T], [Jl Crt, Jl Crr Jl^T]]
    double P[6][6];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            P[i][j] = C[3 + i][3 + j];
            const double v = C[3 + i][0] * Jl[j][0] + C[3 + i][1] * Jl[j][1] + C[3 + i][2] * Jl[j][2];
            P[i][3 + j] = v;
            P[3 + j][i] = v;
        }
    {
        double T[3][3];  // Jl Crr
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) T[i][j] = Jl[i][0] * C[0][j] + Jl[i][1] * C[1][j] + Jl[i][2] * C[2][j];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++) {
                const double v = T[i][0] * Jl[j][0] + T[i][1] * Jl[j][1] + T[i][2] * Jl[j][2];
                P[3 + i][3 + j] = v;
                P[3 + j][3 + i] = v;
            }
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) o->cov_pose[6 * a + b] = P[a][b];
    if constexpr (CAM) {
        // ---- cov_cam_pose = B cov_pose B^T, B = [[Q, W], [0, Q]], Q = -R^T, W = Q [t]x
        double R[9], dummy[27];
        rodrigues_v2m(p, R, dummy, false);
        const double tx = p[3], ty = p[4], tz = p[5];
        const double tX[3][3] = {{0., -tz, ty}, {tz, 0., -tx}, {-ty, tx, 0.}};
        double Q[3][3], W[3][3], X1[3][3], X2[3][3], G[6][6];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Q[i][j] = -R[3 * j + i];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) W[i][j] = Q[i][0] * tX[0][j] + Q[i][1] * tX[1][j] + Q[i][2] * tX[2][j];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                X1[i][j] = Q[i][0] * P[0][j] + Q[i][1] * P[1][j] + Q[i][2] * P[2][j] + W[i][0] * P[3][j] + W[i][1] * P[4][j] + W[i][2] * P[5][j];
                X2[i][j] = Q[i][0] * P[0][3 + j] + Q[i][1] * P[1][3 + j] + Q[i][2] * P[2][3 + j] + W[i][0] * P[3][3 + j] + W[i][1] * P[4][3 + j] +
                           W[i][2] * P[5][3 + j];
            }
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = i; j < 3; j++) {
                const double v = X1[i][0] * Q[j][0] + X1[i][1] * Q[j][1] + X1[i][2] * Q[j][2] + X2[i][0] * W[j][0] + X2[i][1] * W[j][1] + X2[i][2] * W[j][2];
                G[i][j] = v;
                G[j][i] = v;
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double v = X2[i][0] * Q[j][0] + X2[i][1] * Q[j][1] + X2[i][2] * Q[j][2];
                G[i][3 + j] = v;
                G[3 + j][i] = v;
            }
        }
        {
            double T[3][3];  // Q P_rr
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) T[i][j] = Q[i][0] * P[3][3 + j] + Q[i][1] * P[4][3 + j] + Q[i][2] * P[5][3 + j];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = i; j < 3; j++) {
                    const double v = T[i][0] * Q[j][0] + T[i][1] * Q[j][1] + T[i][2] * Q[j][2];
                    G[3 + i][3 + j] = v;
                    G[3 + j][3 + i] = v;
                }
        }
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 6; b++) cov_cam_pose[6 * a + b] = G[a][b];
    }
}

__device__ void pnp_mul3(const double a[9], const double b[9], double d[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// cvUndistortPoints for one pixel: the normalised pinhole point (ox, oy).  Plumb-bob and rational: cvUndistortPointsInternal's five
// fixed-point iterations, always true.  Equidistant: theta_d = |((u - cx) / fx, (v - cy) / fy)|, theta by Newton from theta_d (at most
// ten steps, until |step| < 1e-8), the point = the distorted one times tan(theta) / theta_d; false -- and (ox, oy) the distorted
// point -- where Newton has not converged or theta is not inside [0, PNP_FISHEYE_MAX_THETA): the marker cannot be posed.
template <int MODEL>
__device__ bool pnp_undistort(const double K[9], const double kd[12], double u, double v, double *ox, double *oy)
{
    const double fx = K[0], fy = K[4], ifx = 1. / fx, ify = 1. / fy, cx = K[2], cy = K[5];
    double x = (u - cx) * ifx, y = (v - cy) * ify;
    if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
        const double thd = sqrt(x * x + y * y);
        double th = thd;
        bool ok = false;
        for (int j = 0; j < 10 && !ok; j++) {
            const double th2 = th * th;
            const double f = th * (1 + th2 * (kd[0] + th2 * (kd[1] + th2 * (kd[2] + th2 * kd[3])))) - thd;
            const double df = 1 + th2 * (3 * kd[0] + th2 * (5 * kd[1] + th2 * (7 * kd[2] + th2 * (9 * kd[3]))));
            const double step = f / df;
            th -= step;
            ok = fabs(step) < 1e-8;
        }
        ok = ok && th >= 0. && th < PNP_FISHEYE_MAX_THETA;
        const double sc = (ok && thd > 1e-8) ? tan(th) / thd : 1.;
        *ox = x * sc;
        *oy = y * sc;
        return ok;
    } else {
        const double x0 = x, y0 = y;
        for (int j = 0; j < 5; j++) {
            const double r2 = x * x + y * y;
            double icdist;
            if constexpr (MODEL == FID_CAM_RATIONAL)
                icdist = (1 + ((kd[7] * r2 + kd[6]) * r2 + kd[5]) * r2) / (1 + ((kd[4] * r2 + kd[1]) * r2 + kd[0]) * r2);
            else
                icdist = (1) / (1 + ((kd[4] * r2 + kd[1]) * r2 + kd[0]) * r2);
            if (icdist < 0) {
                x = (u - cx) * ifx;
                y = (v - cy) * ify;
                break;
            }
            double deltaX = 2 * kd[2] * x * y + kd[3] * (r2 + 2 * x * x);
            double deltaY = kd[2] * (r2 + 2 * y * y) + 2 * kd[3] * x * y;
            if constexpr (MODEL == FID_CAM_RATIONAL) {
                deltaX = deltaX + kd[8] * r2 + kd[9] * r2 * r2;
                deltaY = deltaY + kd[10] * r2 + kd[11] * r2 * r2;
            }
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
        *ox = x;
        *oy = y;
        return true;
    }
}

// homography marker plane -> normalised image through the four corners (mnx, mny): unit square (0,0),(1,0),(1,1),(0,1) -> quad
// (Heckbert), composed with (X, Y) -> (X scx + 1/2, 1/2 - Y scy) -- scx = scy = 1 / 2h for the square (-h, h) (h, h) (h, -h)
// (-h, -h), 1 / wx and 1 / wy for a wx x wy rectangle about its centre -- and scaled to h[8] = 1.  False: no such homography.
__device__ __forceinline__ bool pnp_quad_homography(const double mnx[4], const double mny[4], double scx, double scy, double h[9])
{
    const double x0 = mnx[0], y0 = mny[0], x1 = mnx[1], y1 = mny[1], x2 = mnx[2], y2 = mny[2], x3 = mnx[3], y3 = mny[3];
    const double dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
    const double dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
    const double den = dx1 * dy2 - dy1 * dx2;
    if (!(den != 0.)) return false;
    const double gg = (sx * dy2 - sy * dx2) / den, hh = (dx1 * sy - dy1 * sx) / den;
    const double a = x1 - x0 + gg * x1, b = x3 - x0 + hh * x3, c = x0;
    const double d = y1 - y0 + gg * y1, e = y3 - y0 + hh * y3, ff = y0;
    // H = Hunit * [[scx, 0, .5], [0, -scy, .5], [0, 0, 1]]
    h[0] = a * scx;  h[1] = -b * scy;  h[2] = 0.5 * a + 0.5 * b + c;
    h[3] = d * scx;  h[4] = -e * scy;  h[5] = 0.5 * d + 0.5 * e + ff;
    h[6] = gg * scx; h[7] = -hh * scy; h[8] = 0.5 * gg + 0.5 * hh + 1.;
    if (!(h[8] != 0.)) return false;
    const double sc = 1. / h[8];
#pragma unroll
    for (int i = 0; i < 9; i++) h[i] *= sc;
    return true;
}

// rotation and translation from a plane -> normalised-image homography (cvFindExtrinsicCameraParams2, planar branch)
__device__ __forceinline__ void pnp_pose_from_h(double h[9], double t3[3])
{
    const double h1n = sqrt(h[0] * h[0] + h[3] * h[3] + h[6] * h[6]), h2n = sqrt(h[1] * h[1] + h[4] * h[4] + h[7] * h[7]);
    const double s1 = 1. / fmax(h1n, DBL_EPSILON), s2 = 1. / fmax(h2n, DBL_EPSILON), stt = 2. / fmax(h1n + h2n, DBL_EPSILON);
    t3[0] = h[2] * stt; t3[1] = h[5] * stt; t3[2] = h[8] * stt;
    h[0] *= s1; h[3] *= s1; h[6] *= s1;
    h[1] *= s2; h[4] *= s2; h[7] *= s2;
    h[2] = h[3] * h[7] - h[6] * h[4];
    h[5] = h[6] * h[1] - h[0] * h[7];
    h[8] = h[0] * h[4] - h[3] * h[1];
    double rtmp[3], dummy[27];
    rodrigues_m2v(h, rtmp);
    rodrigues_v2m(rtmp, h, dummy, false);
}

// eigenvalues (descending, cv::SVD's order) and eigenvectors (the rows of Vt) of the centred scatter matrix MM (destroyed)
__device__ __forceinline__ void pnp_scatter_eig(double MM[3][3], double W[3], double Vt[3][3])
{
    jacobi3(MM, Vt);
    W[0] = MM[0][0]; W[1] = MM[1][1]; W[2] = MM[2][2];
    // eigenvalues descending, the rows of Vt with them (cv::SVD's order)
#pragma unroll
    for (int i = 0; i < 2; i++) {
        int mx = i;
#pragma unroll
        for (int j = i + 1; j < 3; j++)
            if (W[j] > W[mx]) mx = j;
        if (mx != i) {
            const double t = W[i];
            W[i] = W[mx];
            W[mx] = t;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double u = Vt[i][k];
                Vt[i][k] = Vt[mx][k];
                Vt[mx][k] = u;
            }
        }
    }
}

// the frame of a coplanar set (cvFindExtrinsicCameraParams2, planar branch): Rt turns the points into their plane (the scatter
// matrix's eigenvectors, made right-handed; the identity when the plane is z = const already), tt = -Rt Mc
__device__ __forceinline__ void pnp_plane_frame(const double Vt[3][3], const double Mc[3], double Rt[9], double tt[3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = Vt[i][j];
    if (Rt[2] * Rt[2] + Rt[5] * Rt[5] < 1e-10)
        for (int i = 0; i < 9; i++) Rt[i] = (i % 4 == 0) ? 1. : 0.;
    const double det = Rt[0] * (Rt[4] * Rt[8] - Rt[5] * Rt[7]) - Rt[1] * (Rt[3] * Rt[8] - Rt[5] * Rt[6]) + Rt[2] * (Rt[3] * Rt[7] - Rt[4] * Rt[6]);
    if (det < 0)
        for (int i = 0; i < 9; i++) Rt[i] = -Rt[i];
    for (int i = 0; i < 3; i++) tt[i] = -(Rt[i * 3] * Mc[0] + Rt[i * 3 + 1] * Mc[1] + Rt[i * 3 + 2] * Mc[2]);
}

// the start for a set that is not coplanar: the closed-form pose of ONE marker -- the one the kernel found largest in the image
// -- composed with that marker's place in the set's frame.  c0, c1, c3: its object corners (c2 is not needed), cc: its centre,
// uv: its four image corners.  The marker's frame: x along c0 -> c1, y along c3 -> c0, origin at cc.
template <int MODEL>
__device__ __forceinline__ void pnp_start_largest(const double *c0, const double *c1, const double *c3, const double cc[3], const double (*uv)[2],
                                                  const double K[9], const double kd[12], double param[6])
{
    double ex[3], ey[3], ez[3];
    for (int a = 0; a < 3; a++) {
        ex[a] = c1[a] - c0[a];
        ey[a] = c0[a] - c3[a];
    }
    const double wx = sqrt(ex[0] * ex[0] + ex[1] * ex[1] + ex[2] * ex[2]), wy = sqrt(ey[0] * ey[0] + ey[1] * ey[1] + ey[2] * ey[2]);
    for (int a = 0; a < 3; a++) ex[a] /= wx;
    ez[0] = ex[1] * ey[2] - ex[2] * ey[1]; ez[1] = ex[2] * ey[0] - ex[0] * ey[2]; ez[2] = ex[0] * ey[1] - ex[1] * ey[0];
    const double wz = sqrt(ez[0] * ez[0] + ez[1] * ez[1] + ez[2] * ez[2]);
    for (int a = 0; a < 3; a++) ez[a] /= wz;
    ey[0] = ez[1] * ex[2] - ez[2] * ex[1]; ey[1] = ez[2] * ex[0] - ez[0] * ex[2]; ey[2] = ez[0] * ex[1] - ez[1] * ex[0];
    double mnx[4], mny[4];
    for (int i = 0; i < 4; i++) (void)pnp_undistort<MODEL>(K, kd, uv[i][0], uv[i][1], &mnx[i], &mny[i]);
    double h[9], Rq[9], tq[3];
    for (int i = 0; i < 3; i++) param[3 + i] = 0.;
    if (wx > 0. && wy > 0. && wz > 0. && pnp_quad_homography(mnx, mny, 1. / wx, 1. / wy, h)) {
        pnp_pose_from_h(h, tq);
        // set -> camera: X_cam = Rq B^T (X - centre) + tq, B = [ex ey ez]
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rq[3 * i + j] = h[3 * i] * ex[j] + h[3 * i + 1] * ey[j] + h[3 * i + 2] * ez[j];
        for (int i = 0; i < 3; i++) param[3 + i] = tq[i] - (Rq[3 * i] * cc[0] + Rq[3 * i + 1] * cc[1] + Rq[3 * i + 2] * cc[2]);
    } else {
        for (int i = 0; i < 9; i++) Rq[i] = (i % 4 == 0) ? 1. : 0.;
    }
    rodrigues_m2v(Rq, param);
}

// entry j of the two DLT rows of one correspondence: Lx = {X, Y, 1, 0, 0, 0, -x X, -x Y, -x}, Ly = {0, 0, 0, X, Y, 1, -y X, -y Y, -y}
__device__ __forceinline__ void pnp_dlt_entry(int j, double X, double Y, double x, double y, double *lx, double *ly)
{
    const double b = j % 3 == 0 ? X : (j % 3 == 1 ? Y : 1.0);
    *lx = j < 3 ? b : (j < 6 ? 0.0 : -x * b);
    *ly = j < 3 ? 0.0 : (j < 6 ? b : -y * b);
}

// the eigenvector of the smallest eigenvalue of the symmetric 9 x 9 A (LDS, both triangles filled; destroyed), by cyclic Jacobi in
// LDS: the rotation's angle in every lane, lane k < 9 turns its entries.  V: 81 doubles of LDS, its rows the eigenvectors.  Returns
// the row, the same in every lane.
__device__ int pnp_smallest_eigvec9(double *A, double *V, int lane)
{
    for (int e = lane; e < 81; e += 64) V[e] = (e / 9 == e % 9) ? 1. : 0.;
    SR_LDS_SYNC();
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0;
        for (int p = 0; p < 9; p++)
            for (int q = p + 1; q < 9; q++) off += A[p * 9 + q] * A[p * 9 + q];
        if (!(off >= 1e-300)) break;
        for (int p = 0; p < 9; p++)
            for (int q = p + 1; q < 9; q++) {
                const double apq = A[p * 9 + q];
                if (fabs(apq) < 1e-300) continue;  // (wave-uniform)
                const double app = A[p * 9 + p], aqq = A[q * 9 + q];
                const double theta = (aqq - app) / (2. * apq);
                const double t = (theta >= 0 ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                const double c = 1. / sqrt(t * t + 1.), sn = t * c;
                SR_LDS_SYNC();
                if (lane < 9) {
                    const double akp = A[lane * 9 + p], akq = A[lane * 9 + q];
                    A[lane * 9 + p] = c * akp - sn * akq;
                    A[lane * 9 + q] = sn * akp + c * akq;
                }
                SR_LDS_SYNC();
                if (lane < 9) {
                    const double apk = A[p * 9 + lane], aqk = A[q * 9 + lane];
                    A[p * 9 + lane] = c * apk - sn * aqk;
                    A[q * 9 + lane] = sn * apk + c * aqk;
                    const double vpk = V[p * 9 + lane], vqk = V[q * 9 + lane];
                    V[p * 9 + lane] = c * vpk - sn * vqk;
                    V[q * 9 + lane] = sn * vpk + c * vqk;
                }
                SR_LDS_SYNC();
            }
    }
    int row = 0;
    double wmin = A[0];
    for (int i = 1; i < 9; i++)
        if (A[i * 9 + i] <= wmin) {
            wmin = A[i * 9 + i];
            row = i;
        }
    return row;
}

// the tail of HomographyEstimatorCallback::runKernel (fundam.cpp): LtL is in A (LDS, both triangles); the eigenvector of its
// smallest eigenvalue, de-normalised by the two point sets' centroids (c..) and scales (s..; m: image, M: plane), scaled to
// H[8] = 1.  The ACCUMULATION of LtL is not part of it on purpose: k_stag_bundle_pose sums every entry serially over the points
// on lanes < 45 (sb_homography_dlt), the wave-strided kernels sum strided per-lane partials and butterfly them
// (pnp_homography_dlt below) -- the float sums land on different bits, and each kernel's bits are its result.
__device__ __forceinline__ bool pnp_dlt_finish(double *A, double *V, int lane, double cmx, double cmy, double smx, double smy, double cMx, double cMy,
                                               double sMx, double sMy, double H[9])
{
    const int row = pnp_smallest_eigvec9(A, V, lane);
    double H0[9], T[9];
    for (int i = 0; i < 9; i++) H0[i] = V[row * 9 + i];
    const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
    const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    pnp_mul3(invHnorm, H0, T);
    pnp_mul3(T, Hnorm2, H0);
    if (!(H0[8] != 0)) return false;
    const double sc = 1. / H0[8];
    for (int i = 0; i < 9; i++) H[i] = H0[i] * sc;
    return true;
}

// CvLevMarq (calibration.cpp: cvFindExtrinsicCameraParams2's solver, TermCriteria(20, FLT_EPSILON)) for the six pose parameters,
// restated once: its states (CALC_J: the normal equations at param are there; CHECK_ERR: the error at the moved param is there;
// its STARTED is the caller's first evaluation, with the Jacobian), lambda = 10^lambdaLg10 from -3 kept inside [-16, 16], the retry
// with ten times the damping while the error grows, the stop on the relative step or after 20 accepted steps.  Every lane of a
// group runs the same machine on the same sums.
//     step() is called after every evaluation of the residuals at param -- the first with the Jacobian -- and moves param; true: it
//     needs the residuals at the new param, and with needJ the normal equations S = J^T J (packed upper triangle, solve6_spd's
//     order) and gJ = J^T e as well.  errSq() reduces |e|^2 of the last residuals; it is a callable because CvLevMarq does not read
//     the norm after every evaluation (not after an accepted step past the first), and a reduction that is not read is not made.
//     False: converged, param is the result.
struct LevMarq {
    enum { CALC_J = 2, CHECK_ERR = 3 };
    double prevParam[6], prevErrNorm = 0.;
    int lambdaLg10 = -3, iters = 0, state = CALC_J;
    template <class ErrSq>
    __device__ __forceinline__ bool step(double param[6], const double S[21], const double gJ[6], ErrSq &&errSq, bool &needJ)
    {
        if (state == CALC_J) {
#pragma unroll
            for (int i = 0; i < 6; i++) prevParam[i] = param[i];
            if (iters == 0) prevErrNorm = sqrt(errSq());
            state = CHECK_ERR;
        } else {
            const double errNorm = sqrt(errSq());
            if (!(errNorm > prevErrNorm && ++lambdaLg10 <= 16)) {  // accepted (or the damping is at its end)
                lambdaLg10 = lambdaLg10 - 1 > -16 ? lambdaLg10 - 1 : -16;
                double dn = 0, pn = 0;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    dn += (param[i] - prevParam[i]) * (param[i] - prevParam[i]);
                    pn += prevParam[i] * prevParam[i];
                }
                const double rel = sqrt(dn) / (sqrt(pn) + DBL_EPSILON);
                if (++iters >= 20 || rel < FLT_EPSILON) return false;
                prevErrNorm = errNorm;
                needJ = true;
                state = CALC_J;
                return true;
            }
        }
        // param <- prevParam - (J^T J + lambda diag(J^T J))^-1 J^T e: the first move from prevParam, or the retry with more damping
        double xs[6];
        solve6_spd(S, gJ, lm_lambda(lambdaLg10), xs);
#pragma unroll
        for (int i = 0; i < 6; i++) param[i] = prevParam[i] - xs[i];
        needJ = false;
        return true;
    }
};

// ------------------------------------------------------------------------------------------------ the wave-strided solve
// solvePnP over ONE point set by ONE wave: point p on lane p % 64, per-lane partial sums in point order, one xor butterfly per
// entry -- a fixed order, reproducible from run to run, the same value in every lane.  k_map_pose, k_map_pose_robust and
// k_charuco_pose all sum in this order, so they share the body; each hands its points over as a VIEW of its LDS tables, a small
// struct that is inlined away:
//     PLANAR_ONLY                  (static constexpr bool) the object points are (x, y, 0): no planarity test, no other start
//     obj(i, M)                    object point i as three doubles (a PLANAR_ONLY view: the literal 0. as the third)
//     img(i, c)                    coordinate c of image point i
//     mn(i, c)                     the undistorted image point rounded to float (findHomography's input)
//     Mxy(i)                       the float in-plane point, two floats of LDS written and read in view order
//     A(), V()                     81 doubles of LDS each: the DLT's 9 x 9 and its eigenvectors
//     markers(), area(k)           for the start of a set that is not coplanar: the markers in view order, the image area of
//                                  marker k (a PLANAR_ONLY view has neither, nor what follows)
//     MARKER_IN_PLACE              (static constexpr bool) how the start reads the largest marker: false -- first(k), the index
//                                  of its first point (of four in a row), the points copied into registers through obj / img;
//                                  true -- marker_obj(k), marker_img(k), its four object and image points where they lie in
//                                  LDS.  Same values either way; each kernel has the form it measured faster with (HISTORY)
typedef const double (*PnpObj4)[3];  // four object points in a row
typedef const double (*PnpImg4)[2];  // four image points in a row

// HomographyEstimatorCallback::runKernel (fundam.cpp) over the n correspondences Mxy -> mn of a view, with the float-input
// normalisation; each of the 45 entries of LtL is a strided partial sum per lane and a butterfly.  Every lane returns the same H.
template <class View>
__device__ bool pnp_homography_dlt(const View &v, int n, int lane, double H[9])
{
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    for (int i = lane; i < n; i += 64) {
        cmx += v.mn(i, 0);
        cmy += v.mn(i, 1);
        cMx += v.Mxy(i)[0];
        cMy += v.Mxy(i)[1];
    }
    cmx = wave_sum_f64(cmx) / n; cmy = wave_sum_f64(cmy) / n; cMx = wave_sum_f64(cMx) / n; cMy = wave_sum_f64(cMy) / n;
    for (int i = lane; i < n; i += 64) {
        smx += fabs(v.mn(i, 0) - cmx);
        smy += fabs(v.mn(i, 1) - cmy);
        sMx += fabs(v.Mxy(i)[0] - cMx);
        sMy += fabs(v.Mxy(i)[1] - cMy);
    }
    smx = wave_sum_f64(smx); smy = wave_sum_f64(smy); sMx = wave_sum_f64(sMx); sMy = wave_sum_f64(sMy);
    if (!(fabs(smx) >= DBL_EPSILON) || !(fabs(smy) >= DBL_EPSILON) || !(fabs(sMx) >= DBL_EPSILON) || !(fabs(sMy) >= DBL_EPSILON)) return false;
    smx = n / smx; smy = n / smy; sMx = n / sMx; sMy = n / sMy;
    // LtL, entry (j, k), j <= k: the lane's points in their order, then the butterfly
    double *A = v.A();
    for (int j = 0; j < 9; j++)
        for (int k = j; k < 9; k++) {
            double acc = 0;
            for (int i = lane; i < n; i += 64) {
                const double x = (v.mn(i, 0) - cmx) * smx, y = (v.mn(i, 1) - cmy) * smy;
                const double X = (v.Mxy(i)[0] - cMx) * sMx, Y = (v.Mxy(i)[1] - cMy) * sMy;
                double lxj, lyj, lxk, lyk;
                pnp_dlt_entry(j, X, Y, x, y, &lxj, &lyj);
                pnp_dlt_entry(k, X, Y, x, y, &lxk, &lyk);
                acc += lxj * lxk + lyj * lyk;
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) {
                A[j * 9 + k] = acc;
                A[k * 9 + j] = acc;
            }
        }
    return pnp_dlt_finish(A, v.V(), lane, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
}

// the 2 n residuals of a view at param, residual r (point r / 2, coordinate r % 2) on lane r % 64: returns the lane's share of
// |e|^2, which the caller butterflies when it reads it.  With needJ the normal equations as well, every lane the same: S = J^T J
// (packed upper triangle, solve6_spd's order) and, with GRAD, gJ = J^T e (without: gJ is not touched; the covariance needs S alone).
template <int MODEL, bool GRAD, class View>
__device__ __forceinline__ double pnp_wave_residuals(const View &v, int n, int lane, const double K[9], const double kd[12], const double param[6],
                                                     bool needJ, double S[21], double gJ[6])
{
    const int nres = 2 * n;
    double Sp[21], gp[6], e2 = 0;
    for (int i = 0; i < 21; i++) Sp[i] = 0.;
    for (int i = 0; i < 6; i++) gp[i] = 0.;
    for (int r = lane; r < nres; r += 64) {
        const int p = r >> 1, sel = r & 1;
        double M[3], Jrow[6];
        v.obj(p, M);
        const double err = project_one<MODEL>(M, param, K, kd, sel, Jrow, needJ) - v.img(p, sel);
        e2 += err * err;
        if (needJ) {
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int c = a; c < 6; c++) Sp[idx++] += Jrow[a] * Jrow[c];
                if constexpr (GRAD) gp[a] += Jrow[a] * err;
            }
        }
    }
    if (needJ) {
#pragma unroll
        for (int i = 0; i < 21; i++) S[i] = wave_sum_f64(Sp[i]);
        if constexpr (GRAD) {
#pragma unroll
            for (int i = 0; i < 6; i++) gJ[i] = wave_sum_f64(gp[i]);
        }
    }
    return e2;
}

// cv::solvePnP (ITERATIVE) over the n points of a view and getReprojectionError over them; every lane returns the same param and
// image_error.  The caller has made its LDS tables visible to the wave (SR_LDS_SYNC) and may call again with another view of them.
//   (a) planarity: cvFindExtrinsicCameraParams2's test, the eigenvalues of the centred scatter matrix.
//   (b) the start.  Coplanar: the points turned into their plane, the DLT homography over all of them.  Not coplanar: the closed-form
//       pose of the marker with the largest image area (the first of equals in view order) composed with that marker's place in the
//       set (OpenCV runs a 12 x 12 DLT there; the start is unpinned).
//   (c) CvLevMarq with the camera model's distortion in the projection and its Jacobian.
//   (d) the reprojection error: projections rounded to float (vector<Point2f>), sum |d|^2 / n.
// A PLANAR_ONLY view sums the scatter matrix over x and y and turns the points with two terms: the three-term forms with z = 0. give
// another sign to a zero in corner cases (-0. + 0.) and cost instructions that nothing folds without fast-math.
template <int MODEL, class View>
__device__ __forceinline__ void pnp_wave_solve(const View &v, int n, int lane, const double K[9], const double kd[12], double param[6],
                                               double *image_error)
{
    // ---- (a) the centred scatter matrix of the object points and its eigenvalues and eigenvectors
    double Mc[3] = {0, 0, 0}, W[3], Vt[3][3];
    bool planar = true;
    if constexpr (View::PLANAR_ONLY) {
        for (int p = lane; p < n; p += 64) {
            double M[3];
            v.obj(p, M);
            Mc[0] += M[0];
            Mc[1] += M[1];
        }
        for (int a = 0; a < 2; a++) Mc[a] = wave_sum_f64(Mc[a]) / n;
        double m3[3] = {0, 0, 0};
        for (int p = lane; p < n; p += 64) {
            double M[3];
            v.obj(p, M);
            const double d0 = M[0] - Mc[0], d1 = M[1] - Mc[1];
            m3[0] += d0 * d0; m3[1] += d0 * d1; m3[2] += d1 * d1;
        }
        for (int i = 0; i < 3; i++) m3[i] = wave_sum_f64(m3[i]);
        double MM[3][3] = {{m3[0], m3[1], 0.}, {m3[1], m3[2], 0.}, {0., 0., 0.}};
        pnp_scatter_eig(MM, W, Vt);
    } else {
        for (int p = lane; p < n; p += 64) {
            double M[3];
            v.obj(p, M);
            for (int a = 0; a < 3; a++) Mc[a] += M[a];
        }
        for (int a = 0; a < 3; a++) Mc[a] = wave_sum_f64(Mc[a]) / n;
        double m6[6] = {0, 0, 0, 0, 0, 0};
        for (int p = lane; p < n; p += 64) {
            double M[3];
            v.obj(p, M);
            const double d[3] = {M[0] - Mc[0], M[1] - Mc[1], M[2] - Mc[2]};
            m6[0] += d[0] * d[0]; m6[1] += d[0] * d[1]; m6[2] += d[0] * d[2];
            m6[3] += d[1] * d[1]; m6[4] += d[1] * d[2]; m6[5] += d[2] * d[2];
        }
        for (int i = 0; i < 6; i++) m6[i] = wave_sum_f64(m6[i]);
        double MM[3][3] = {{m6[0], m6[1], m6[2]}, {m6[1], m6[3], m6[4]}, {m6[2], m6[4], m6[5]}};
        pnp_scatter_eig(MM, W, Vt);
        planar = W[2] / W[1] < 1e-3;
    }
    // ---- (b) the start
    for (int i = 0; i < 6; i++) param[i] = 0.;
    if (planar) {
        double Rt[9], tt[3];
        pnp_plane_frame(Vt, Mc, Rt, tt);
        SR_LDS_SYNC();  // (a solve before this one has read its Mxy)
        for (int p = lane; p < n; p += 64) {
            double M[3];
            v.obj(p, M);
            if constexpr (View::PLANAR_ONLY) {
                v.Mxy(p)[0] = (float)(Rt[0] * M[0] + Rt[1] * M[1] + tt[0]);
                v.Mxy(p)[1] = (float)(Rt[3] * M[0] + Rt[4] * M[1] + tt[1]);
            } else {
                v.Mxy(p)[0] = (float)(Rt[0] * M[0] + Rt[1] * M[1] + Rt[2] * M[2] + tt[0]);
                v.Mxy(p)[1] = (float)(Rt[3] * M[0] + Rt[4] * M[1] + Rt[5] * M[2] + tt[1]);
            }
        }
        SR_LDS_SYNC();
        double h[9], R[9];
        if (pnp_homography_dlt(v, n, lane, h)) {
            double t3[3];
            pnp_pose_from_h(h, t3);
            for (int i = 0; i < 3; i++) param[3 + i] = h[i * 3] * tt[0] + h[i * 3 + 1] * tt[1] + h[i * 3 + 2] * tt[2] + t3[i];
            pnp_mul3(h, Rt, R);
        } else {
            for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1. : 0.;
        }
        rodrigues_m2v(R, param);
    } else if constexpr (!View::PLANAR_ONLY) {
        // the marker with the largest image area, the first of equals: per lane over its markers, then a butterfly on (area, index)
        const int nmk = v.markers();
        int big = lane < nmk ? lane : 0;
        double abig = v.area(big);
        for (int k = lane + 64; k < nmk; k += 64)
            if (v.area(k) > abig) {
                abig = v.area(k);
                big = k;
            }
        for (int mask = 1; mask < 64; mask <<= 1) {
            const double ao = shfl_xor_f64(abig, mask);
            const int bo = __shfl_xor(big, mask, WAVE);
            if (ao > abig || (ao == abig && bo < big)) {
                abig = ao;
                big = bo;
            }
        }
        // its four object and image points: where they lie in LDS, or copied into registers through the view's accessors
        double cq[4][3], uvq[4][2];
        PnpObj4 c = cq;
        PnpImg4 uv = uvq;
        if constexpr (View::MARKER_IN_PLACE) {
            c = v.marker_obj(big);
            uv = v.marker_img(big);
        } else {
            const int p0 = v.first(big);
            for (int q = 0; q < 4; q++) {
                v.obj(p0 + q, cq[q]);
                uvq[q][0] = v.img(p0 + q, 0);
                uvq[q][1] = v.img(p0 + q, 1);
            }
        }
        const double cc[3] = {0.5 * (c[0][0] + c[2][0]), 0.5 * (c[0][1] + c[2][1]), 0.5 * (c[0][2] + c[2][2])};
        pnp_start_largest<MODEL>(c[0], c[1], c[3], cc, uv, K, kd, param);
    }
    // ---- (c) CvLevMarq over the 2 n residuals
    double S[21], gJ[6], e2 = 0;
    bool needJ = true;
    LevMarq lm;
    do {
        e2 = pnp_wave_residuals<MODEL, true>(v, n, lane, K, kd, param, needJ, S, gJ);
    } while (lm.step(param, S, gJ, [&] { return wave_sum_f64(e2); }, needJ));
    // ---- (d) getReprojectionError
    double tot = 0;
    for (int p = lane; p < n; p += 64) {
        double M[3], Jrow[6];
        v.obj(p, M);
        const double dx = v.img(p, 0) - (double)(float)project_one<MODEL>(M, param, K, kd, 0, Jrow, false);
        const double dy = v.img(p, 1) - (double)(float)project_one<MODEL>(M, param, K, kd, 1, Jrow, false);
        const double e = sqrt(dx * dx + dy * dy);
        tot += e * e;
    }
    *image_error = wave_sum_f64(tot) / n;
}

// the pose part of a record (fid_map_pose_out, fid_charuco_pose_out: rvec, tvec, R, cam_R, cam_t, image_error; the counts in front
// of them are the kernel's): param as the board's pose in the camera frame and, inverted, the camera's in the board's ...
template <class Rec>
__device__ __forceinline__ void pnp_pose_record(Rec &o, const double param[6], double image_error)
{
    for (int i = 0; i < 3; i++) {
        o.rvec[i] = param[i];
        o.tvec[i] = param[3 + i];
    }
    double dummy[27];
    rodrigues_v2m(param, o.R, dummy, false);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) o.cam_R[3 * i + j] = o.R[3 * j + i];
        o.cam_t[i] = -(o.R[i] * param[3] + o.R[3 + i] * param[4] + o.R[6 + i] * param[5]);
    }
    o.image_error = image_error;
}
// ... and the record of a set that has no pose: all zero, image_error as the caller's exit defines it
template <class Rec>
__device__ __forceinline__ void pnp_pose_record_zero(Rec &o, double image_error)
{
    for (int i = 0; i < 3; i++) o.rvec[i] = o.tvec[i] = o.cam_t[i] = 0.;
    for (int i = 0; i < 9; i++) o.R[i] = o.cam_R[i] = 0.;
    o.image_error = image_error;
}
