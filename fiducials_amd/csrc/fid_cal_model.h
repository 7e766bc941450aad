// fid_cal_model.h -- the residual function of the joint solves (fid_calib.hip: camera calibration; fid_map_build.hip: building the map)
// and its derivatives, on fid_pnp.h.  Moved here from fid_calib.hip as it stood, so that both files include what they use.
#pragma once
#include "fid_pnp.h"

// index of (a, b), a <= b, in the packed upper triangle of an N x N matrix, row-major
__device__ __forceinline__ int cal_tri(int a, int b, int N) { return a * N - a * (a - 1) / 2 + (b - a); }

// THE RESIDUAL FUNCTION of the calibration, in the arithmetic of its NumPy restatement (tests/calib_restatement.py: rodrigues, distort,
// project): the rotation as I + sin(th) [k]x + (1 - cos(th)) [k]x^2 with k = r / th, the pinhole point by a division, the radial
// polynomials by Horner's rule, the rational model's quotient as one division.  In a weakly determined problem (a valley of the
// cost) the minimiser moves by 1e-7 .. 1e-6 standard deviations with every rounding that the residual function makes differently, so
// the function the device minimises is the stated one, expression by expression, not fid_pnp.h's project_one (cvProjectPoints2's
// expressions: multiplication by 1 / z, powers of r2, 1 / denominator) -- the two agree to a few ulps and have the same derivatives.
__device__ __forceinline__ void cal_rotation_value(const double rv[3], double R[9])
{
    const double th = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    if (th < DBL_EPSILON) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1. : 0.;
        return;
    }
    double sn, cs;
    sincos(th, &sn, &cs);
    const double k0 = rv[0] / th, k1 = rv[1] / th, k2 = rv[2] / th, c1 = 1. - cs;
    const double kx[9] = {0., -k2, k1, k2, 0., -k0, -k1, k0, 0.};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double kk = kx[3 * i] * kx[j] + kx[3 * i + 1] * kx[3 + j] + kx[3 * i + 2] * kx[6 + j];
            R[3 * i + j] = ((i == j ? 1. : 0.) + sn * kx[3 * i + j]) + c1 * kk;
        }
}
// the pinhole point (x, y) of object point M under (R, t); *iz = 1 / z for the derivatives (z = 0: the point as it is, as project_one)
__device__ __forceinline__ void cal_pinhole(const double M[3], const double *R, const double t[3], double *x, double *y, double *iz)
{
    const double xc = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + t[0];
    const double yc = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + t[1];
    const double zc = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + t[2];
    *x = zc ? xc / zc : xc;
    *y = zc ? yc / zc : yc;
    *iz = zc ? 1. / zc : 1.;
}
// the plumb-bob / rational model's distorted point; *q: the radial factor, *iden: 1 / its denominator (1 for plumb-bob)
template <int MODEL>
__device__ __forceinline__ void cal_distort(double x, double y, const double k[12], double r2, double *xd, double *yd, double *q, double *iden)
{
    double cd = 1. + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
    *iden = 1.;
    if constexpr (MODEL == FID_CAM_RATIONAL) {
        const double den = 1. + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
        cd = cd / den;
        *iden = 1. / den;
    }
    double u = x * cd + 2. * k[2] * x * y + k[3] * (r2 + 2. * x * x);
    double v = y * cd + k[2] * (r2 + 2. * y * y) + 2. * k[3] * x * y;
    if constexpr (MODEL == FID_CAM_RATIONAL) {
        u = u + r2 * (k[8] + r2 * k[9]);
        v = v + r2 * (k[10] + r2 * k[11]);
    }
    *xd = u;
    *yd = v;
    *q = cd;
}
// one residual's projection without derivatives (k_calib_eval): cal_row's value, the same expressions
template <int MODEL>
__device__ __forceinline__ double cal_project(const double M[3], const double *R, const double t[3], const double K[9], const double k[12], int sel)
{
    double x, y, iz;
    cal_pinhole(M, R, t, &x, &y, &iz);
    const bool su = sel == 0;
    if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
        const double r2 = x * x + y * y, r = sqrt(r2);
        const double th = atan(r), th2 = th * th;
        const double thd = th * (1 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3]))));
        const double scale = !(r > 1e-8) ? 1. : thd / r;
        return su ? K[0] * (x * scale) + K[2] : K[4] * (y * scale) + K[5];
    } else {
        double xd, yd, q, iden;
        cal_distort<MODEL>(x, y, k, x * x + y * y, &xd, &yd, &q, &iden);
        return su ? xd * K[0] + K[2] : yd * K[4] + K[5];
    }
}

// rodrigues_v2m (fid_pnp.h: cvRodrigues2 vector -> matrix with dR / dr, J[9 i + k] = dR_k / dr_i) for ONE wave-uniform rotation vector,
// spread over the lanes: the derivative's expressions are the same, but its 27 entries are made by 27 lanes from small tables in LDS
// (tmp: 80 doubles) instead of by every lane in 100-odd registers.  out[0..8] = R (cal_rotation_value's), out[9..35] = J.
__device__ __forceinline__ void cal_rotation_lds(const double *__restrict__ rv, double *out, double *tmp, int lane)
{
    double rx = rv[0], ry = rv[1], rz = rv[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {  // (wave-uniform)
        if (lane < 36) {
            double val = 0.;
            if (lane < 9) val = (lane % 4 == 0) ? 1. : 0.;
            const int e = lane - 9;
            if (e == 5 || e == 15 || e == 19) val = -1.;
            if (e == 7 || e == 11 || e == 21) val = 1.;
            out[lane] = val;
        }
        SR_LDS_SYNC();
        return;
    }
    double c, sn;
    sincos(theta, &sn, &c);
    const double c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    if (lane == 0) {
        // tmp: rrt[9] | r_x[9] | drrt[27] | d_r_x_[27] | the unit axis [3]
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
        const double drrt[27] = {rx + rx, ry, rz, ry, 0,       0,  rz, 0,  0,       0, rx, 0, rx, ry + ry,
                                 rz,      0,  rz, 0,  0,       0,  rx, 0,  0,       ry, rx, ry, rz + rz};
        const double d_r_x_[27] = {0, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 9; k++) {
            tmp[k] = rrt[k];
            tmp[9 + k] = r_x[k];
        }
#pragma unroll
        for (int k = 0; k < 27; k++) {
            tmp[18 + k] = drrt[k];
            tmp[45 + k] = d_r_x_[k];
        }
        tmp[72] = rx;
        tmp[73] = ry;
        tmp[74] = rz;
    }
    SR_LDS_SYNC();
    if (lane == 0) {  // (R is the residual function's: cal_rotation_value, what k_calib_eval computes)
        double R[9];
        cal_rotation_value(rv, R);
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = R[k];
    } else if (lane >= 9 && lane < 36) {
        const int e = lane - 9, i = e / 9, k = e % 9;
        const double ri = tmp[72 + i];
        const double a0 = -sn * ri, a1 = (sn - 2 * c1 * itheta) * ri, a2 = c1 * itheta;
        const double a3 = (c - sn * itheta) * ri, a4 = sn * itheta;
        out[lane] = a0 * ((k % 4 == 0) ? 1. : 0.) + a1 * tmp[k] + a2 * tmp[18 + e] + a3 * tmp[9 + k] + a4 * tmp[45 + e];
    }
    SR_LDS_SYNC();
}

// One residual's projection with its whole Jacobian row: cal_project<MODEL>'s value (the same expressions in the same order) for the
// object point M under the pose whose rotation R and dR / d rvec (rodrigues_v2m's J) lie in LDS and whose translation is t; Jp[0..5] =
// d / d(rvec, tvec) by the chain rule through the distortion's own 2 x 2 Jacobian (gx, gy: the derivatives of the selected distorted
// coordinate with respect to the pinhole point), d[0..15] = d / d(fx fy cx cy D[0..11]), zero where the model has no such slot.
// Reading R and dR from LDS as they are needed keeps the 36 doubles of a pose out of every lane's registers.
template <int MODEL>
__device__ __forceinline__ double cal_row(const double M[3], const double *R, const double *dR, const double t[3], const double K[9], const double k[12],
                                           int sel, double Jp[6], double d[16])
{
    const double X = M[0], Y = M[1], Z = M[2];
    double x, y, z;  // (z: 1 / depth)
    cal_pinhole(M, R, t, &x, &y, &z);
    const bool su = sel == 0;
    const double f = su ? K[0] : K[4], c = su ? x : y;
#pragma unroll
    for (int i = 0; i < 16; i++) d[i] = 0.;
    d[2] = su ? 1. : 0.;
    d[3] = su ? 0. : 1.;
    double out, gx, gy;
    if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
        const double r2 = x * x + y * y, r = sqrt(r2);
        const double th = atan(r), th2 = th * th;
        const double poly = 1 + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3])));
        const double thd = th * poly;
        const bool tiny = !(r > 1e-8);
        const double scale = tiny ? 1. : thd / r;
        out = su ? K[0] * (x * scale) + K[2] : K[4] * (y * scale) + K[5];
        // d scale = g (x dx + y dy), as in project_one
        const double dpoly = 1 + th2 * (3 * k[0] + th2 * (5 * k[1] + th2 * (7 * k[2] + th2 * (9 * k[3]))));
        const double g = tiny ? 0. : (dpoly / (1 + r2) - scale) / r2;
        gx = (su ? scale : 0.) + c * g * x;
        gy = (su ? 0. : scale) + c * g * y;
        d[0] = su ? x * scale : 0.;
        d[1] = su ? 0. : y * scale;
        // d theta_d / d k_i = theta^(2 i + 3); the scale is theta_d / r
        const double gk = tiny ? 0. : f * c / r;
        const double t3 = th * th2, t5 = t3 * th2, t7 = t5 * th2, t9 = t7 * th2;
        d[4] = gk * t3;
        d[5] = gk * t5;
        d[6] = gk * t7;
        d[7] = gk * t9;
    } else {
        const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
        double xd, yd, q, icdist2;  // q = numerator / denominator, icdist2 = 1 / denominator
        cal_distort<MODEL>(x, y, k, r2, &xd, &yd, &q, &icdist2);
        out = su ? xd * K[0] + K[2] : yd * K[4] + K[5];
        // the derivative of q by r2; the prism's derivative by r2 for the selected coordinate
        double dq = (k[0] + 2 * k[1] * r2 + 3 * k[4] * r4) * icdist2, dpr = 0.;
        if constexpr (MODEL == FID_CAM_RATIONAL) {
            dq -= q * icdist2 * (k[5] + 2 * k[6] * r2 + 3 * k[7] * r4);
            dpr = su ? k[8] + 2 * k[9] * r2 : k[10] + 2 * k[11] * r2;
        }
        const double w = 2 * (c * dq + dpr);  // times x, y: through r2
        gx = w * x + (su ? q + 2 * k[2] * y + 6 * k[3] * x : 2 * k[2] * x + 2 * k[3] * y);
        gy = w * y + (su ? 2 * k[2] * x + 2 * k[3] * y : q + 6 * k[2] * y + 2 * k[3] * x);
        d[0] = su ? xd : 0.;
        d[1] = su ? 0. : yd;
        const double fc = f * c * icdist2;
        d[4] = fc * r2;                  // k1
        d[5] = fc * r4;                  // k2
        d[6] = f * (su ? a1 : a3);       // p1
        d[7] = f * (su ? a2 : a1);       // p2
        d[8] = fc * r6;                  // k3
        if constexpr (MODEL == FID_CAM_RATIONAL) {
            const double g = -fc * q;  // d/d k4..k6 of c numerator / (1 + k4 r2 + k5 r4 + k6 r6)
            d[9] = g * r2;
            d[10] = g * r4;
            d[11] = g * r6;
            d[12] = su ? f * r2 : 0.;    // s1 s2: u only
            d[13] = su ? f * r4 : 0.;
            d[14] = su ? 0. : f * r2;    // s3 s4: v only
            d[15] = su ? 0. : f * r4;
        }
    }
    // the pinhole point by the translation: dx = (z, 0, -x z), dy = (0, z, -y z); by the rotation: z (dX - x dZ), z (dY - y dZ)
    const double fgx = f * gx, fgy = f * gy;
    Jp[3] = fgx * z;
    Jp[4] = fgy * z;
    Jp[5] = -(fgx * x + fgy * y) * z;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double *q9 = dR + 9 * j;
        const double dX = X * q9[0] + Y * q9[1] + Z * q9[2], dY = X * q9[3] + Y * q9[4] + Z * q9[5], dZ = X * q9[6] + Y * q9[7] + Z * q9[8];
        Jp[j] = z * (fgx * (dX - x * dZ) + fgy * (dY - y * dZ));
    }
    return out;
}


