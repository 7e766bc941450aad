// fid_stag_pose.hip -- STag rows s9, s10: pose refinement (ellipse fit + simplex search) and the 5-point marker pose.
// Part of the fid_stag.hip translation unit (included there; not compiled on its own).
// ------------------------------------------------------------------------------------------------ K16: pose refinement
// PoseRefiner::refineMarkerPose (PoseRefiner.cpp:12-190), one wave per marker:
//   (1) pick the edge segment that is the image of the marker's circular border: a closed loop of >= 20 pixels inside the
//       quad whose back-projection stays within 0.1 of the circle of radius 0.4 and whose distances to 36 points of that circle
//       sum to < 1.8 (lanes take pixels; minima are order-free, the sum over the 36 points runs in order);
//   (2) fit an ellipse to it: customEllipse(pix*, n) (Ellipse.cpp:296-473) = Fitzgibbon's direct least squares through the
//       reference's own small linear algebra (scatter matrix summed in pixel order -- one lane per matrix entry --, choldc,
//       Gauss-Jordan inverse, Jacobi eigenvalues, all 1-based like the original);
//   (3) move the 9 entries of H with Nelder-Mead so that H^T C H is the circle (0.5, 0.5, r 0.4): cv::DownhillSolver with its
//       defaults, restated (see oracle/stag_ref.cpp for the same restatement on the checker's side); cost Refine::calc (:224-258);
//   (4) corners and centre from the new H.
// The reference takes atan / sin / cos of the ellipse's rotation from glibc; here the sine and cosine come from the tangent
// algebraically (sr_conic_to_ellipse): the results agree to rounding, the optimiser then follows a path that can differ in the
// last bits -- this row's parity bar is a tolerance (corners to 1e-3 px), not equality.
struct SrEllipse {
    double A1, B1, C1, D1, E1, F1, cX, cY, a, b;
};

// the conic -> ellipse conversion shared by both customEllipse constructors (Ellipse.cpp:394-454, :668-728); coefficients
// come in unnormalised
__device__ void sr_conic_to_ellipse(double A1, double B1, double C1, double D1, double E1, double F1, SrEllipse *e)
{
    B1 /= A1; C1 /= A1; D1 /= A1; E1 /= A1; F1 /= A1; A1 /= A1;
    double A2, C2, D2, E2, F2, sr = 0, cr = 1;  // (the reference leaves rotation unset when B1 == 0)
    bool rotated = false;
    if (B1 == 0) {
        A2 = A1; C2 = C1; D2 = D1; E2 = E1; F2 = F1;
    } else {
        // rotation = atan(t) / 2 with t = B1 / (A1 - C1); the reference takes cos / sin of 2 * rotation and of rotation from libm.
        // Here they come from t itself: cos(atan t) = 1 / sqrt(1 + t^2), sin(atan t) = t / sqrt(1 + t^2), and the half angle
        // (|rotation| <= pi / 4: its cosine is positive) cos r = sqrt((1 + cos 2r) / 2), sin r = sin 2r / (2 cos r) -- two square
        // roots and three divisions instead of an arctangent and two sincos calls (~ 380 of the ~ 950 dependent f64
        // instructions of one cost evaluation; the simplex search is a chain of a few hundred of them).  Equal to the libm road
        // to rounding, like the device's atan / sin / cos were: this row's parity bar is the tolerance stated above.
        const double t = B1 / (A1 - C1);
        double s2, c2;
        if (fabs(t) > 1e150) {  // A1 == C1 (t infinite: 2 r = +- pi / 2), or t * t would overflow
            c2 = 0.0;
            s2 = copysign(1.0, t);
        } else {
            c2 = 1.0 / sqrt(1.0 + t * t);
            s2 = t * c2;
        }
        cr = sqrt(0.5 * (1.0 + c2));
        sr = s2 / (2.0 * cr);
        rotated = t != 0.0;  // (rotation != 0)
        A2 = 0.5 * (A1 * (1 + c2 + B1 * s2 + C1 * (1 - c2)));
        C2 = 0.5 * (A1 * (1 - c2 - B1 * s2 + C1 * (1 + c2)));
        D2 = D1 * cr + E1 * sr;
        E2 = -D1 * sr + E1 * cr;
        F2 = F1;
    }
    const double D3 = D2 / A2, E3 = E2 / C2;
    double cX = -(D3 / 2), cY = -(E3 / 2);
    const double F3 = A2 * (cX * cX) + C2 * (cY * cY) - F2;
    e->a = sqrt(F3 / A2);
    e->b = sqrt(F3 / C2);
    if (rotated) {
        const double tx = cX, ty = cY;
        cX = tx * cr - ty * sr;
        cY = tx * sr + ty * cr;
    }
    e->cX = cX; e->cY = cY;
    e->A1 = A1; e->B1 = B1; e->C1 = C1; e->D1 = D1; e->E1 = E1; e->F1 = F1;
}

// 1-based 7 x 7 scratch matrices as in the reference
typedef double SrM[7][7];

__device__ void sr_jacobi(SrM a, double d[7], SrM v)
{
    const int n = 6;
    double b[7], z[7];
    for (int ip = 1; ip <= n; ip++) {
        for (int iq = 1; iq <= n; iq++) v[ip][iq] = 0.0;
        v[ip][ip] = 1.0;
    }
    for (int ip = 1; ip <= n; ip++) {
        b[ip] = d[ip] = a[ip][ip];
        z[ip] = 0.0;
    }
    auto rot = [](SrM m, int i, int j, int k, int l, double tau, double s) {
        const double g = m[i][j], h = m[k][l];
        m[i][j] = g - s * (h + g * tau);
        m[k][l] = h + s * (g - h * tau);
    };
    for (int i = 1; i <= 50; i++) {
        double sm = 0.0;
        for (int ip = 1; ip <= n - 1; ip++)
            for (int iq = ip + 1; iq <= n; iq++) sm += fabs(a[ip][iq]);
        if (sm == 0.0) return;
        const double tresh = i < 4 ? 0.2 * sm / (n * n) : 0.0;
        for (int ip = 1; ip <= n - 1; ip++) {
            for (int iq = ip + 1; iq <= n; iq++) {
                const double g = 100.0 * fabs(a[ip][iq]);
                if (i > 4 && g == 0.0) a[ip][iq] = 0.0;
                else if (fabs(a[ip][iq]) > tresh) {
                    double h = d[iq] - d[ip], t;
                    if (g == 0.0) t = (a[ip][iq]) / h;
                    else {
                        const double theta = 0.5 * h / (a[ip][iq]);
                        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                        if (theta < 0.0) t = -t;
                    }
                    const double c = 1.0 / sqrt(1 + t * t), sn = t * c, tau = sn / (1.0 + c);
                    h = t * a[ip][iq];
                    z[ip] -= h; z[iq] += h; d[ip] -= h; d[iq] += h;
                    a[ip][iq] = 0.0;
                    for (int j = 1; j <= ip - 1; j++) rot(a, j, ip, j, iq, tau, sn);
                    for (int j = ip + 1; j <= iq - 1; j++) rot(a, ip, j, j, iq, tau, sn);
                    for (int j = iq + 1; j <= n; j++) rot(a, ip, j, iq, j, tau, sn);
                    for (int j = 1; j <= n; j++) rot(v, j, ip, j, iq, tau, sn);
                }
            }
        }
        for (int ip = 1; ip <= n; ip++) {
            b[ip] += z[ip];
            d[ip] = b[ip];
            z[ip] = 0.0;
        }
    }
}

// customEllipse(pix*, n) from the scatter matrix S (1-based, full) on: returns false if the inverse fails
__device__ bool sr_fit_from_scatter(SrM S, SrEllipse *e)
{
    const int n = 6;
    SrM L, invL, temp, C, V, sol, Const;
    double d[7], p[7];
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) L[i][j] = invL[i][j] = temp[i][j] = C[i][j] = V[i][j] = sol[i][j] = Const[i][j] = 0.0;
    for (int i = 0; i < 7; i++) d[i] = p[i] = 0.0;
    Const[1][3] = -2; Const[2][2] = 1; Const[3][1] = -2;  // FPF mode
    // choldc
    for (int i = 1; i <= n; i++) {
        for (int j = i; j <= n; j++) {
            double sum = S[i][j];
            for (int k = i - 1; k >= 1; k--) sum -= S[i][k] * S[j][k];
            if (i == j) {
                if (sum > 0.0) p[i] = sqrt(sum);
            } else
                S[j][i] = sum / p[i];
        }
    }
    for (int i = 1; i <= n; i++)
        for (int j = i; j <= n; j++) {
            if (i == j) L[i][i] = p[i];
            else {
                L[j][i] = S[j][i];
                L[i][j] = 0.0;
            }
        }
    // inverse(L): Gauss-Jordan with row pivoting on [L | I]
    {
        double A[7][14];
        for (int k = 0; k < 7; k++)
            for (int j = 0; j < 14; j++) A[k][j] = 0.0;
        for (int k = 1; k <= n; k++) {
            for (int j = 1; j <= n; j++) A[k][j] = L[k][j];  // (column n + 1 stays 0 as in the reference)
            A[k][k - 1 + n + 2] = 1;
        }
        for (int k = 1; k <= n; k++) {
            double maxpivot = fabs(A[k][k]);
            int npivot = k;
            for (int i = k; i <= n; i++)
                if (maxpivot < fabs(A[i][k])) {
                    maxpivot = fabs(A[i][k]);
                    npivot = i;
                }
            if (!(maxpivot >= 10e-20)) return false;
            if (npivot != k)
                for (int j = k; j <= 2 * n + 1; j++) {
                    const double t = A[npivot][j];
                    A[npivot][j] = A[k][j];
                    A[k][j] = t;
                }
            const double Dv = A[k][k];
            for (int j = 2 * n + 1; j >= k; j--) A[k][j] = A[k][j] / Dv;
            for (int i = 1; i <= n; i++)
                if (i != k) {
                    const double mult = A[i][k];
                    for (int j = 2 * n + 1; j >= k; j--) A[i][j] = A[i][j] - mult * A[k][j];
                }
        }
        for (int k = 1; k <= n; k++)
            for (int j = n + 2, q = 1; j <= 2 * n + 1; j++, q++) invL[k][q] = A[k][j];
    }
    // temp = Const * invL^T, C = invL * temp
    for (int pp = 1; pp <= n; pp++)
        for (int q = 1; q <= n; q++) {
            temp[pp][q] = 0.0;
            for (int l = 1; l <= n; l++) temp[pp][q] = temp[pp][q] + Const[pp][l] * invL[q][l];
        }
    for (int pp = 1; pp <= n; pp++)
        for (int q = 1; q <= n; q++) {
            C[pp][q] = 0.0;
            for (int l = 1; l <= n; l++) C[pp][q] = C[pp][q] + invL[pp][l] * temp[l][q];
        }
    sr_jacobi(C, d, V);
    // sol = invL^T * V
    for (int pp = 1; pp <= n; pp++)
        for (int q = 1; q <= n; q++) {
            sol[pp][q] = 0.0;
            for (int l = 1; l <= n; l++) sol[pp][q] = sol[pp][q] + invL[l][pp] * V[l][q];
        }
    for (int j = 1; j <= n; j++) {
        double mod = 0.0;
        for (int i = 1; i <= n; i++) mod += sol[i][j] * sol[i][j];
        for (int i = 1; i <= n; i++) sol[i][j] /= sqrt(mod);
    }
    int solind = 0;
    for (int i = 1; i <= n; i++)
        if (d[i] < 0 && fabs(d[i]) > 10e-20) solind = i;
    sr_conic_to_ellipse(sol[1][solind], sol[2][solind], sol[3][solind], sol[4][solind], sol[5][solind], sol[6][solind], e);
    return true;
}

// cv::Mat::inv() of a 3 x 3 (closed form, as OpenCV's invert() does for n <= 3)
__device__ void sr_inv3(const double S[9], double D[9])
{
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    for (int k = 0; k < 9; k++) D[k] = 0.0;
    if (d != 0.) {
        d = 1. / d;
        D[0] = (S[4] * S[8] - S[5] * S[7]) * d; D[1] = (S[2] * S[7] - S[1] * S[8]) * d; D[2] = (S[1] * S[5] - S[2] * S[4]) * d;
        D[3] = (S[5] * S[6] - S[3] * S[8]) * d; D[4] = (S[0] * S[8] - S[2] * S[6]) * d; D[5] = (S[2] * S[3] - S[0] * S[5]) * d;
        D[6] = (S[3] * S[7] - S[4] * S[6]) * d; D[7] = (S[1] * S[6] - S[0] * S[7]) * d; D[8] = (S[0] * S[4] - S[1] * S[3]) * d;
    }
}

// Refine::calc (PoseRefiner.cpp:224-258): x[i + 3 j] = H(i, j)
__device__ double sr_cost(const double x[9], const double Cm[9])
{
    double H[9], HT[9], T[9], P[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            H[3 * i + j] = x[i + j * 3];
            HT[3 * j + i] = x[i + j * 3];
        }
    pnp_mul3(HT, Cm, T);
    pnp_mul3(T, H, P);
    SrEllipse e;
    sr_conic_to_ellipse(P[0], -P[1] * 2, P[4], P[2] * 2, -P[5] * 2, P[8], &e);
    double acc = 0;
    acc += fabs(e.a - 0.4);
    acc += fabs(e.b - 0.4);
    acc += fabs(e.cX - 0.5);
    acc += fabs(-e.cY - 0.5);
    return acc;
}

// Refine::calc for FOUR points at once, one per 16-lane row of the wave (round 4).  One evaluation is ~900 dependent f64
// instructions when a lane does it alone, and the solver's three candidates of an iteration kept three lanes of 64 busy: the
// wave issued the whole stream for them (4 300 cycles per iteration, 4.8 cycles per instruction -- the single-wave issue rate
// tools/valu_calib.hip measures).  Here a ROW works on one point:
//   lane (a, b) = 4 a + b of the row (a, b < 3) forms T[a][b] = sum_k H[k][a] C[k][b], takes T[a][0..2] from its quad by DPP
//   quad_perm and forms P[a][b] = sum_k T[a][k] H[k][b] -- the two 3 x 3 products in 2 x 5 instructions instead of 2 x 45;
//   the lanes that hold P00, P01, P11, P02, P12, P22 make the conic coefficients and divide by A1 in ONE division; the rest of
//   Ellipse.cpp's conversion runs on lane pairs: one lane the A / D / x / a side, its neighbour the C / E / y / b side (the two
//   sides are the same expressions with other operands and signs: D3 = D2 / A2 beside E3 = E2 / C2, sqrt(F3 / A2) beside
//   sqrt(F3 / C2)), exchanging by quad_perm.
// Every quantity is formed by the same operations on the same operands, in the same order, as sr_cost (a - b is taken as
// a + (-b), which is the same IEEE result); the cost comes back in every lane of the row.  -DSR_COST_SCALAR keeps sr_cost.
__device__ __forceinline__ double sr_row_from(double v, int lane_in_row, int lane)
{
    return shfl_f64(v, (lane & 48) | lane_in_row);
}
__device__ double sr_cost_rows(const double xa[3], const double xb[3], const double cmb[3], int lane)
{
    const int r = lane & 15, a = r >> 2, b = r & 3;
    // T[a][b], then the row a of T from the quad, then P[a][b]  (pnp_mul3's expression: a0 b0 + a1 b1 + a2 b2)
    const double T = xa[0] * cmb[0] + xa[1] * cmb[1] + xa[2] * cmb[2];
    const double t0 = dpp_f64<0x00>(T), t1 = dpp_f64<0x55>(T), t2 = dpp_f64<0xAA>(T);
    const double Pab = t0 * xb[0] + t1 * xb[1] + t2 * xb[2];
    // the conic of sr_conic_to_ellipse(P0, -2 P1, P4, 2 P2, -2 P5, P8): this lane's coefficient, unnormalised
    double coef = Pab;                       // A1 (lane 0), C1 (lane 5), F1 (lane 10)
    if (r == 1 || r == 6) coef = -Pab * 2;   // B1 = -P[1] * 2 (lane 1), E1 = -P[5] * 2 (lane 6)
    if (r == 2) coef = Pab * 2;              // D1 = P[2] * 2
    const double A1raw = sr_row_from(coef, 0, lane);
    const double q = coef / A1raw;           // B1 /= A1 ... F1 /= A1, A1 /= A1: one division for all six
    const double A1 = sr_row_from(q, 0, lane), B1 = sr_row_from(q, 1, lane), C1 = sr_row_from(q, 5, lane), D1 = sr_row_from(q, 2, lane),
                 E1 = sr_row_from(q, 6, lane), F1 = sr_row_from(q, 10, lane);
    const bool side = (r & 1) != 0;          // false: the A2 / D / x / a side, true: the C2 / E / y / b side
    double V2, W2, F2, sr = 0, cr = 1;       // V2 = A2 | C2, W2 = D2 | E2
    bool rotated = false;
    if (B1 == 0) {
        V2 = side ? C1 : A1;
        W2 = side ? E1 : D1;
        F2 = F1;
    } else {
        const double t = B1 / (A1 - C1);
        double s2, c2;
        if (fabs(t) > 1e150) {
            c2 = 0.0;
            s2 = copysign(1.0, t);
        } else {
            c2 = 1.0 / sqrt(1.0 + t * t);
            s2 = t * c2;
        }
        cr = sqrt(0.5 * (1.0 + c2));
        sr = s2 / (2.0 * cr);
        rotated = t != 0.0;
        // A2 = 0.5 (A1 (1 + c2 + B1 s2 + C1 (1 - c2))), C2 = 0.5 (A1 (1 - c2 - B1 s2 + C1 (1 + c2)))
        const double sc2 = side ? -c2 : c2, bs = B1 * s2, sbs = side ? -bs : bs;
        V2 = 0.5 * (A1 * (1 + sc2 + sbs + C1 * (1 - sc2)));
        // D2 = D1 cr + E1 sr, E2 = -D1 sr + E1 cr
        W2 = (side ? -D1 : D1) * (side ? sr : cr) + E1 * (side ? cr : sr);
        F2 = F1;
    }
    const double W3 = W2 / V2;               // D3 = D2 / A2 beside E3 = E2 / C2
    double cc = -(W3 / 2);                   // cX | cY
    const double term = V2 * (cc * cc);      // A2 cX^2 | C2 cY^2
    const double oterm = dpp_f64<0xB1>(term);
    const double F3 = (side ? oterm + term : term + oterm) - F2;
    const double ax = sqrt(F3 / V2);         // a | b
    if (rotated) {
        const double occ = dpp_f64<0xB1>(cc);
        // cX = tx cr - ty sr (this lane holds tx), cY = tx sr + ty cr (this lane holds ty)
        cc = side ? occ * sr + cc * cr : cc * cr - occ * sr;
    }
    const double e_ax = fabs(ax - 0.4);                               // |a - 0.4| | |b - 0.4|
    const double e_c = side ? fabs(-cc - 0.5) : fabs(cc - 0.5);       // |cX - 0.5| | |-cY - 0.5|
    const double o_ax = dpp_f64<0xB1>(e_ax), o_c = dpp_f64<0xB1>(e_c);
    double acc = 0;
    acc += side ? o_ax : e_ax;
    acc += side ? e_ax : o_ax;
    acc += side ? o_c : e_c;
    acc += side ? e_c : o_c;
    return sr_row_from(acc, 0, lane);
}

// cv::DownhillSolver::minimize with the default TermCriteria(MAX_ITER + EPS, 5000, 1e-6), 9 dimensions, run by one wave with
// the simplex in LDS.  The three candidate points of an iteration -- reflection (-1), expansion (-2), contraction (0.5) --
// depend only on the current simplex: lanes 0, 1, 2 evaluate them side by side and the solver's decision sequence then
// picks what it would have evaluated one after the other (the evaluation counter advances as in the sequential solver).
// The ten vertices of the start simplex and of a shrink step are evaluated by ten lanes.  Same arithmetic per point as the
// sequential form (column sums in vertex order, the same alpha / beta expressions).
// wave-wide min / max of doubles on DPP row operations (fid_kernels.hip: FID_DPP_SCAN_STEPS), the result in every lane
__device__ __forceinline__ double sr_wave_min_f64(double v)
{
    unsigned long long u = __double_as_longlong(v);
    unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
#define S_(C, M)                                                                                              \
    {                                                                                                         \
        const unsigned ol = (unsigned)FID_DPP(0, (int)lo, C, M), oh = (unsigned)FID_DPP(0x7ff00000, (int)hi, C, M); \
        const double o = __longlong_as_double(((unsigned long long)oh << 32) | ol);                           \
        const double m = fmin(__longlong_as_double(((unsigned long long)hi << 32) | lo), o);                  \
        const unsigned long long mu = __double_as_longlong(m);                                                \
        lo = (unsigned)mu;                                                                                    \
        hi = (unsigned)(mu >> 32);                                                                            \
    }
    FID_DPP_SCAN_STEPS(S_)  // (+inf fills the lanes a step does not reach)
#undef S_
    lo = (unsigned)__builtin_amdgcn_readlane((int)lo, 63);
    hi = (unsigned)__builtin_amdgcn_readlane((int)hi, 63);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double sr_wave_max_nonneg_f64(double v)  // v >= 0 in every lane
{
    unsigned long long u = __double_as_longlong(v);
    unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
#define S_(C, M)                                                                                    \
    {                                                                                               \
        const unsigned ol = (unsigned)FID_DPP(0, (int)lo, C, M), oh = (unsigned)FID_DPP(0, (int)hi, C, M); \
        const double o = __longlong_as_double(((unsigned long long)oh << 32) | ol);                 \
        const double m = fmax(__longlong_as_double(((unsigned long long)hi << 32) | lo), o);        \
        const unsigned long long mu = __double_as_longlong(m);                                      \
        lo = (unsigned)mu;                                                                          \
        hi = (unsigned)(mu >> 32);                                                                  \
    }
    FID_DPP_SCAN_STEPS(S_)
#undef S_
    lo = (unsigned)__builtin_amdgcn_readlane((int)lo, 63);
    hi = (unsigned)__builtin_amdgcn_readlane((int)hi, 63);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

struct SrSimplex {
    double p[10][9], y[10], sum[9];
};

__device__ void sr_downhill(double x[9], const double step[9], const double Cm[9], int lane, SrSimplex *S, int *evals = nullptr)
{
    const int nd = 9;
    if (lane <= nd) {
        for (int j = 0; j < nd; j++) {
            double v = x[j];
            if (lane == 0) v -= 0.5 * step[j];
            else if (lane - 1 == j) v += 0.5 * step[j];
            S->p[lane][j] = v;
        }
    }
    SR_LDS_SYNC();
#ifdef SR_COST_SCALAR
    auto eval_rows = [&](int skip) {  // y[i] = f(p[i]) for every vertex but `skip`, one lane per vertex
        const int i = lane <= nd ? lane : nd;
        double row[9];
        for (int j = 0; j < nd; j++) row[j] = S->p[i][j];
        const double v = sr_cost(row, Cm);
        if (lane <= nd && lane != skip) S->y[lane] = v;
        SR_LDS_SYNC();
    };
#else
    // the lane's place in its row's two 3 x 3 products (sr_cost_rows) and the column b of C it multiplies with
    const int ra = ((lane & 15) >> 2) < 3 ? (lane & 15) >> 2 : 2, rb = (lane & 3) < 3 ? lane & 3 : 2;
    const double cmb[3] = {rb == 0 ? Cm[0] : rb == 1 ? Cm[1] : Cm[2], rb == 0 ? Cm[3] : rb == 1 ? Cm[4] : Cm[5],
                           rb == 0 ? Cm[6] : rb == 1 ? Cm[7] : Cm[8]};
    auto eval_rows = [&](int skip) {  // y[i] = f(p[i]) for every vertex but `skip`: four vertices at a time, a 16-lane row each
        for (int v0 = 0; v0 <= nd; v0 += 4) {
            const int i = v0 + (lane >> 4) <= nd ? v0 + (lane >> 4) : nd;
            double xa[3], xb[3];
            for (int k = 0; k < 3; k++) {
                xa[k] = S->p[i][3 * ra + k];
                xb[k] = S->p[i][3 * rb + k];
            }
            const double v = sr_cost_rows(xa, xb, cmb, lane);
            if ((lane & 15) == 0 && v0 + (lane >> 4) <= nd && i != skip) S->y[i] = v;
        }
        SR_LDS_SYNC();
    };
#endif
    // column sums in vertex order, and in the same pass over the column its extent |max - min| (the termination test's range,
    // round 5: it read the ten vertices a second time at the top of every iteration)
    double col_range = 0;  // (lanes >= nd carry 0)
    auto update_sum = [&]() {
        if (lane < nd) {
            double acc = 0., mn = INFINITY, mx = -INFINITY;
            for (int i = 0; i <= nd; i++) {
                const double v = S->p[i][lane];
                acc += v;
                mn = fmin(mn, v);
                mx = fmax(mx, v);
            }
            S->sum[lane] = acc;
            col_range = fabs(mx - mn);
        }
        SR_LDS_SYNC();
    };
    auto replace_point = [&](int ihi, double alpha_, double ytry) {
        // (alpha_ is one of -1, -2, 0.5: the quotient is one of three constants, no division per iteration)
        const double alpha = alpha_ == -1.0 ? (1.0 - -1.0) / 9 : alpha_ == -2.0 ? (1.0 - -2.0) / 9 : (1.0 - alpha_) / nd, beta = alpha - alpha_;
        // (a lane reads back only its own column: what it has just written is there without a synchronisation in between)
        if (lane < nd) S->p[ihi][lane] = S->sum[lane] * alpha - S->p[ihi][lane] * beta;
        if (lane == 0) S->y[ihi] = ytry;
        update_sum();
    };
    // the candidate a lane's row works on: reflection (-1), expansion (-2), contraction (0.5) -- its two coefficients, once
    const double row_a = (lane >> 4) == 0 ? -1.0 : (lane >> 4) == 1 ? -2.0 : 0.5;
    const double row_alpha = (1.0 - row_a) / nd, row_beta = row_alpha - row_a;
    int fcount = nd + 1;
    eval_rows(-1);
    update_sum();
    for (;;) {
        // (round 5) lowest, highest and next-highest vertex by RANK: lane i < 10 holds y[i] and counts the vertices above it; when
        // the highest, the second highest and the lowest value each occur once -- ten function values of ten different points:
        // always, bar a degenerate start -- the solver's scan below has exactly these three answers (strict comparisons find the
        // one maximum and the one second maximum whatever the order, `<=` the one minimum), and they cost ten compares in all
        // lanes at once instead of the scan's thirty compare-and-select chains (150 of an iteration's 1 000 instructions).
        int ilo = 0, ihi = 0, inhi = 0;
        double v_lo = 0, v_hi = 0, v_nhi = 0;
        bool ranked;
        {
            const double yl = S->y[lane < 10 ? lane : 9];
            int above = 0;
#pragma unroll
            for (int j = 0; j <= 9; j++) above += bcast_f64(yl, j) > yl ? 1 : 0;
            const unsigned m0 = (unsigned)__ballot(lane < 10 && above == 0), m1 = (unsigned)__ballot(lane < 10 && above == 1),
                           m9 = (unsigned)__ballot(lane < 10 && above == 9);
            ranked = __builtin_popcount(m0) == 1 && __builtin_popcount(m1) == 1 && __builtin_popcount(m9) == 1;
            if (ranked) {
                ihi = __builtin_ctz(m0); inhi = __builtin_ctz(m1); ilo = __builtin_ctz(m9);
                v_hi = bcast_f64(yl, ihi); v_nhi = bcast_f64(yl, inhi); v_lo = bcast_f64(yl, ilo);
            }
        }
        if (!ranked) {
        double y[10];
#pragma unroll
        for (int i = 0; i <= 9; i++) y[i] = S->y[i];
        // the solver's scan for the lowest, highest and next-highest vertex -- the same comparisons in the same order, with the
        // VALUES y[ilo], y[ihi], y[inhi] carried beside the indices: indexing the register array y[] with a run-time index costs
        // a ten-way select chain per read, thirty of them per scan (the scan was about half of an iteration's 5 700 cycles)
        ilo = 0;
        v_lo = y[0];
        if (y[0] > y[1]) { ihi = 0; inhi = 1; v_hi = y[0]; v_nhi = y[1]; } else { ihi = 1; inhi = 0; v_hi = y[1]; v_nhi = y[0]; }
#pragma unroll
        for (int i = 0; i <= 9; i++) {
            const double yv = y[i];
            if (yv <= v_lo) { ilo = i; v_lo = yv; }
            if (yv > v_hi) { inhi = ihi; v_nhi = v_hi; ihi = i; v_hi = yv; }
            else if (yv > v_nhi && i != ihi) { inhi = i; v_nhi = yv; }
        }
        if (ilo == inhi || ilo == ihi) {
            bool found = false;
#pragma unroll
            for (int i = 0; i <= 9; i++)
                if (!found && y[i] == v_lo && i != ihi && i != inhi) { ilo = i; found = true; }
        }
        }
        const double error = fabs(v_hi - v_lo);
        double range = 0;
        {
            const double r = col_range;
            // (lanes >= nd carry 0: the maximum of the first 16-lane row is the wave's -- four DPP steps instead of six)
            {
                unsigned long long u = __double_as_longlong(r);
                unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
#define S_(C)                                                                                       \
    {                                                                                               \
        const unsigned ol = (unsigned)FID_DPP(0, (int)lo, C, 0xf), oh = (unsigned)FID_DPP(0, (int)hi, C, 0xf); \
        const double o = __longlong_as_double(((unsigned long long)oh << 32) | ol);                 \
        const double m = fmax(__longlong_as_double(((unsigned long long)hi << 32) | lo), o);        \
        const unsigned long long mu = __double_as_longlong(m);                                      \
        lo = (unsigned)mu;                                                                          \
        hi = (unsigned)(mu >> 32);                                                                  \
    }
                S_(0x111) S_(0x112) S_(0x114) S_(0x118)  // row_shr:1, 2, 4, 8: lane 15 holds the maximum of lanes 0..15
#undef S_
                lo = (unsigned)__builtin_amdgcn_readlane((int)lo, 15);
                hi = (unsigned)__builtin_amdgcn_readlane((int)hi, 15);
                range = __longlong_as_double(((unsigned long long)hi << 32) | lo);
            }
        }
        if (range <= 0.000001 || error <= 0.000001 || fcount >= 5000) {
            for (int j = 0; j < nd; j++) x[j] = S->p[ilo][j];
            if (evals) *evals = fcount;
            return;
        }
        const double y_lo = v_lo, y_nhi = v_nhi, y_hi = v_hi;
#ifdef SR_COST_SCALAR
        double buf[9];
        {
            const double a_ = lane == 0 ? -1.0 : lane == 1 ? -2.0 : 0.5;
            const double alpha = (1.0 - a_) / nd, beta = alpha - a_;
            for (int j = 0; j < nd; j++) buf[j] = S->sum[j] * alpha - S->p[ihi][j] * beta;
        }
        const double yl = sr_cost(buf, Cm);
        const double y_refl = bcast_f64(yl, 0), y_exp = bcast_f64(yl, 1), y_con = bcast_f64(yl, 2);
#else
        // row 0: reflection (-1), row 1: expansion (-2), rows 2 and 3: contraction (0.5); a lane forms the six entries it multiplies
        double xa[3], xb[3];
        {
            const double alpha = row_alpha, beta = row_beta;
            for (int k = 0; k < 3; k++) {
                xa[k] = S->sum[3 * ra + k] * alpha - S->p[ihi][3 * ra + k] * beta;
                xb[k] = S->sum[3 * rb + k] * alpha - S->p[ihi][3 * rb + k] * beta;
            }
        }
        const double yl = sr_cost_rows(xa, xb, cmb, lane);
        const double y_refl = bcast_f64(yl, 0), y_exp = bcast_f64(yl, 16), y_con = bcast_f64(yl, 32);
#endif
        fcount++;
        double alpha = -1.0, y_alpha = y_refl;
        if (y_alpha < y_nhi) {
            if (y_alpha < y_lo) {
                fcount++;
                if (y_exp < y_alpha) { alpha = -2.0; y_alpha = y_exp; }
            }
            replace_point(ihi, alpha, y_alpha);
        } else {
            fcount++;
            if (y_con < y_hi) replace_point(ihi, 0.5, y_con);
            else {
                if (lane <= nd && lane != ilo)
                    for (int j = 0; j < nd; j++) S->p[lane][j] = 0.5 * (S->p[lane][j] + S->p[ilo][j]);
                SR_LDS_SYNC();
                eval_rows(ilo);
                fcount += nd;
                update_sum();
            }
        }
    }
}

// PoseRefiner::checkIfPointInQuad (PoseRefiner.cpp:200-222)
__device__ bool sr_in_quad(const double c[8], double px, double py)
{
    const double c1c2x = c[2] - c[0], c1c2y = c[3] - c[1], c1c4x = c[6] - c[0], c1c4y = c[7] - c[1];
    const double c3c2x = c[2] - c[4], c3c2y = c[3] - c[5], c3c4x = c[6] - c[4], c3c4y = c[7] - c[5];
    const double c1px = px - c[0], c1py = py - c[1], c3px = px - c[4], c3py = py - c[5];
    if (sq_cross(c1px, c1py, c1c2x, c1c2y) * sq_cross(c1px, c1py, c1c4x, c1c4y) >= 0) return false;
    if (sq_cross(c1c2x, c1c2y, c1px, c1py) * sq_cross(c1c2x, c1c2y, c1c4x, c1c4y) <= 0) return false;
    if (sq_cross(c3px, c3py, c3c2x, c3c2y) * sq_cross(c3px, c3py, c3c4x, c3c4y) >= 0) return false;
    if (sq_cross(c3c2x, c3c2y, c3px, c3py) * sq_cross(c3c2x, c3c2y, c3c4x, c3c4y) <= 0) return false;
    return true;
}

struct k_stag_refine_fn {
    static constexpr int kBounds = 64;
    __device__ __forceinline__ void operator()(fid_stag_marker *__restrict__ markers, const int *__restrict__ nmarkers,
                                               const int2 *__restrict__ vsegs, const int *__restrict__ nsegs, const int2 *__restrict__ pix,
                                               int *__restrict__ chosen_out) const
    {
        const int m = blockIdx.x, lane = threadIdx.x;
        if (m >= *nmarkers) return;
        fid_stag_marker M = markers[m];
        const double sinVals[36] = {0.000000,  0.173648,  0.342020,  0.500000,  0.642788,  0.766044,  0.866025,  0.939693,  0.984808,
                                    1.000000,  0.984808,  0.939693,  0.866025,  0.766044,  0.642788,  0.500000,  0.342020,  0.173648,
                                    0.000000,  -0.173648, -0.342020, -0.500000, -0.642788, -0.766044, -0.866025, -0.939693, -0.984808,
                                    -1.000000, -0.984808, -0.939693, -0.866025, -0.766044, -0.642788, -0.500000, -0.342020, -0.173648};
        double Hinv[9];
        sr_inv3(M.H, Hinv);
#ifdef SR_TIMING
        const unsigned long long t_0 = __builtin_readcyclecounter();
        int d_cands = 0;
#endif
        // ---- (1) the edge segment of the circular border
        int chosen = -1;
        double minAcc = INFINITY;
        const int ns = *nsegs;
        for (int sg0 = 0; sg0 < ns; sg0 += 64) {
          // the cheap tests (length, closed loop, sampled pixels inside the quad) for 64 segments at once, one per lane; the
          // survivors are then examined one after the other, in segment order, by the whole wave
          unsigned long long cand;
          {
            const int sgl = sg0 + lane;
            bool ok = false;
            if (sgl < ns) {
                const int first = vsegs[sgl].x, n = vsegs[sgl].y;
                if (n >= 20) {
                    const int2 *p = pix + first;
                    if (!(sq_dist2((double)p[0].y, (double)p[0].x, (double)p[n - 1].y, (double)p[n - 1].x) > 7.0 * 7.0)) {
                        ok = true;
                        for (int k = 0; k < n && ok; k += 20)
                            if (!sr_in_quad(M.corners, (double)p[k].y, (double)p[k].x)) ok = false;
                    }
                }
            }
            cand = __ballot(ok);
          }
          while (cand) {
            const int sg = sg0 + __builtin_ctzll(cand);
            cand &= cand - 1;
#ifdef SR_TIMING
            d_cands++;
#endif
            const int first = vsegs[sg].x, n = vsegs[sg].y;
            const int2 *p = pix + first;
            // back-projection; per sample point the minimum over the pixels, per pixel the minimum over the sample points
            bool bad = false;
            // (round 3) first only the per-pixel test that rejects: 22 of the 23 closed loops inside a marker are code dots whose
            // pixels lie nowhere near the circle -- they end here, after the first 64 pixels, without the 36 wave-wide minima per
            // chunk that only the accepted segment's error sum needs (same distances, same comparisons, same decision)
            for (int k0 = 0; k0 < n && !bad; k0 += 64) {
                const int k = k0 + lane;
                const bool act = k < n;
                double pixErr = INFINITY;
                if (act) {
                    const double ex = p[k].y, ey = p[k].x;
                    const double a0 = Hinv[0] * ex + Hinv[1] * ey + Hinv[2] * 1, a1 = Hinv[3] * ex + Hinv[4] * ey + Hinv[5] * 1;
                    const double a2 = Hinv[6] * ex + Hinv[7] * ey + Hinv[8] * 1;
                    const double qx = a0 / a2, qy = a1 / a2;
                    // (round 4) min_s sqrt(x_s) == sqrt(min_s x_s) bit for bit -- the correctly rounded square root is monotone -- so the
                    // rejecting pass takes ONE square root per pixel instead of 36 (23 code-dot loops per marker end in this pass)
                    double m2 = INFINITY;
                    for (int s = 0; s < 36; s++) {
                        const double sx = 0.5 + 0.4 * sinVals[(s + 9) % 36], sy = 0.5 + 0.4 * sinVals[s];
                        const double d2 = (qx - sx) * (qx - sx) + (qy - sy) * (qy - sy);
                        if (d2 < m2) m2 = d2;
                    }
                    pixErr = sqrt(m2);
                }
                if (__ballot(act && pixErr > 0.1)) bad = true;
            }
            if (bad) continue;
            double sampleErr[36];
            for (int s = 0; s < 36; s++) sampleErr[s] = INFINITY;
            for (int k0 = 0; k0 < n; k0 += 64) {
                const int k = k0 + lane;
                double qx = 0, qy = 0;
                const bool act = k < n;
                if (act) {
                    const double ex = p[k].y, ey = p[k].x;
                    const double a0 = Hinv[0] * ex + Hinv[1] * ey + Hinv[2] * 1, a1 = Hinv[3] * ex + Hinv[4] * ey + Hinv[5] * 1;
                    const double a2 = Hinv[6] * ex + Hinv[7] * ey + Hinv[8] * 1;
                    qx = a0 / a2;
                    qy = a1 / a2;
                }
                double pixErr = INFINITY;
                for (int s = 0; s < 36; s++) {
                    const double sx = 0.5 + 0.4 * sinVals[(s + 9) % 36], sy = 0.5 + 0.4 * sinVals[s];
                    const double d = act ? sqrt((qx - sx) * (qx - sx) + (qy - sy) * (qy - sy)) : INFINITY;
                    if (d < pixErr) pixErr = d;
                    const double mn = sr_wave_min_f64(d);
                    if (mn < sampleErr[s]) sampleErr[s] = mn;
                }
                if (__ballot(act && pixErr > 0.1)) bad = true;
            }
            if (bad) continue;
            double errSum = 0;
            for (int s = 0; s < 36; s++) errSum += sampleErr[s];
            if (errSum < minAcc && errSum < 36 * 0.05) {
                minAcc = errSum;
                chosen = sg;
            }
          }
        }
        if (lane == 0) chosen_out[m] = chosen;
        if (chosen < 0) return;
#ifdef SR_TIMING
        const unsigned long long t_1 = __builtin_readcyclecounter();
#endif
        // ---- (2) ellipse through the chosen segment: scatter matrix, one lane per entry (p <= q), summed in pixel order
        __shared__ double s_S[7][7];
        {
            const int first = vsegs[chosen].x, n = vsegs[chosen].y;
            const int2 *p = pix + first;
            if (lane < 49) s_S[lane / 7][lane % 7] = 0.0;
            __builtin_amdgcn_wave_barrier();
            // (round 3) the pixels across the lanes, every lane the 21 running sums of its pixels, then 21 wave sums: the terms are
            // integers (pixel coordinates), so up to ~600 pixels every partial sum is exact in a double whatever the order; beyond
            // that the order changes the last bit of a sum that the ellipse fit and the simplex search, a tolerance row anyway
            // (1e-3 px against the reference), do not resolve.  (One lane per matrix entry walked all n pixels: 0.15 ms per marker.)
            double acc[21];
#pragma unroll
            for (int e = 0; e < 21; e++) acc[e] = 0.0;
            for (int l = lane; l < n; l += 64) {
                const double tx = (double)p[l].y, ty = (double)(-p[l].x);
                const double Dl[6] = {tx * tx, tx * ty, ty * ty, tx, ty, 1.0};
                int e = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++) acc[e++] += Dl[a] * Dl[b];
            }
            {
                int e = 0;
#pragma unroll
                for (int a = 1; a <= 6; a++)
#pragma unroll
                    for (int b = a; b <= 6; b++) {
                        double v = acc[e++];
                        v += shfl_xor_f64(v, 1);
                        v += shfl_xor_f64(v, 2);
                        v += shfl_xor_f64(v, 4);
                        v += shfl_xor_f64(v, 8);
                        v += shfl_xor_f64(v, 16);
                        v += shfl_xor_f64(v, 32);
                        if (lane == 0) {
                            s_S[a][b] = v;
                            s_S[b][a] = v;
                        }
                    }
            }
            __builtin_amdgcn_wave_barrier();
            if (n < 6) return;
        }
        // from here on every lane carries the same values (the fit is small scalar work; the simplex search spreads its function
        // evaluations over the lanes)
        __shared__ SrSimplex s_simplex;
        SrM S;
        for (int i = 0; i < 7; i++)
            for (int j = 0; j < 7; j++) S[i][j] = s_S[i][j];
        SrEllipse E;
        if (!sr_fit_from_scatter(S, &E)) return;
        double Cm[9];
        Cm[0] = E.A1; Cm[1] = Cm[3] = -E.B1 / 2; Cm[4] = E.C1; Cm[2] = Cm[6] = E.D1 / 2; Cm[5] = Cm[7] = -E.E1 / 2; Cm[8] = E.F1;
        // ---- (3) Nelder-Mead over the entries of H
        double x[9], step[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) x[i + j * 3] = M.H[3 * i + j];
        for (int k = 0; k < 9; k++) step[k] = fabs(0.001 * x[k]);
#ifdef SR_TIMING
        const unsigned long long t_2 = __builtin_readcyclecounter();
        int d_evals = 0;
        sr_downhill(x, step, Cm, lane, &s_simplex, &d_evals);
        if (lane == 0)
            printf("refine marker %d: segments %d, candidates examined %d, chosen length %d; ticks: search %llu, scatter + fit %llu, simplex %llu (%d evaluations)\n", m, ns,
                   d_cands, vsegs[chosen].y, t_1 - t_0, t_2 - t_1, (unsigned long long)__builtin_readcyclecounter() - t_2, d_evals);
#else
        sr_downhill(x, step, Cm, lane, &s_simplex);
#endif
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) M.H[3 * i + j] = x[i + j * 3];
        // ---- (4) points from the refined H
        auto project = [&](double px, double py, double *ox, double *oy) {
            const double a0 = M.H[0] * px + M.H[1] * py + M.H[2] * 1, a1 = M.H[3] * px + M.H[4] * py + M.H[5] * 1, a2 = M.H[6] * px + M.H[7] * py + M.H[8] * 1;
            *ox = a0 / a2;
            *oy = a1 / a2;
        };
        project(0.5, 0.5, &M.center[0], &M.center[1]);
        project(0, 0, &M.corners[0], &M.corners[1]);
        project(1, 0, &M.corners[2], &M.corners[3]);
        project(1, 1, &M.corners[4], &M.corners[5]);
        project(0, 1, &M.corners[6], &M.corners[7]);
        if (lane == 0) markers[m] = M;
    }
};

// ------------------------------------------------------------------------------------------------ K17: marker pose
// StagNode::imageCallback -> Common::solvePnpSingle (stag_detect.cpp:140-165, common.hpp:34-46): cv::solvePnP (ITERATIVE) on
// FIVE coplanar points, the marker centre (0, 0, 0) and the four corners (-h, h) (h, h) (h, -h) (-h, -h), h = float(marker_size /
// 2).  Same scheme as the aruco pose kernel (fid_kernels.hip K8), from the same library (fid_pnp.h): closed-form start from the
// four corners, then the reference's Levenberg-Marquardt (LevMarq) on the reprojection error of all five points with
// distortion; a 16-lane group per marker, lane g < 10 owns residual g, the sums by grp_sum16.  Tolerance row (the reference
// starts from a 5-point DLT + refinement; both land on the same minimum).
// COV: the covariance tail behind the result write (fid_abi.h: "pose covariance"; k_stag_pose_cov): one more Jacobian at the returned
// pose, J^T J and |e|^2 by this kernel's grp_sum16, then pnp_covariance in the group's first lane
template <int MODEL, bool COV = false>
__device__ __forceinline__ void k_stag_pose_impl(const fid_stag_marker *__restrict__ markers, const int *__restrict__ nmarkers, PoseCam cam,
                                                  double marker_size, fid_stag_pose_out *__restrict__ out, double sigma_px = 0.,
                                                  fid_pose_cov *__restrict__ cov = nullptr)
{
    const int item = blockIdx.x * 4 + (threadIdx.x >> 4), g = threadIdx.x & 15;
    if (item >= *nmarkers) return;  // group-uniform
    const fid_stag_marker mk = markers[item];
    const double *K = cam.K, *kd = cam.D;
    const float halff = (float)(marker_size / 2.0);
    const double hx = (double)halff;
    const bool act = g < 10;
    const int pi = act ? g >> 1 : 0, sel = g & 1;
    // object point of this lane: 0 centre, 1..4 corners
    double M[3] = {0., 0., 0.};
    if (pi >= 1) {
        M[0] = (pi == 2 || pi == 3) ? hx : -hx;
        M[1] = (pi <= 2) ? hx : -hx;
    }
    const double mobs = pi == 0 ? mk.center[sel] : mk.corners[2 * (pi - 1) + sel];
    // ---- the start: closed form through the four corners
    double param[6] = {0, 0, 0, 0, 0, 0};
    {
        double mnx[4], mny[4], h[9];
        bool posable = true;  // (group-uniform: every lane undistorts all four corners)
        for (int i = 0; i < 4; i++) {
            const bool ok = pnp_undistort<MODEL>(K, kd, mk.corners[2 * i], mk.corners[2 * i + 1], &mnx[i], &mny[i]);
            if constexpr (MODEL == FID_CAM_EQUIDISTANT) posable = posable && ok;
        }
        if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
            double cxn, cyn;
            posable = pnp_undistort<MODEL>(K, kd, mk.center[0], mk.center[1], &cxn, &cyn) && posable;
            if (!posable) {  // a point beyond the model (fid_abi.h: "a marker that cannot be posed"): the documented record
                if (g == 0) {
                    fid_stag_pose_out o;
                    o.id = mk.id;
                    for (int i = 0; i < 3; i++) o.rvec[i] = o.tvec[i] = 0.;
                    for (int i = 0; i < 9; i++) o.R[i] = 0.;
                    out[item] = o;
                    if constexpr (COV) pnp_cov_zero(cov + item, 1, 5, nullptr);
                }
                return;
            }
        }
        const double sc0 = 1. / (2. * hx);
        if (pnp_quad_homography(mnx, mny, sc0, sc0, h)) {
            pnp_pose_from_h(h, param + 3);
        } else {
            for (int i = 0; i < 9; i++) h[i] = (i % 4 == 0) ? 1. : 0.;
        }
        rodrigues_m2v(h, param);
    }
    // ---- CvLevMarq over the 10 residuals, the sums over the marker's sixteen lanes
    double S[21], gJ[6], Jrow[6] = {0, 0, 0, 0, 0, 0}, err = 0;
    bool needJ = true;
    LevMarq lm;
    do {
        const double pr = project_one<MODEL>(M, param, K, kd, sel, Jrow, needJ);
        err = act ? pr - mobs : 0.;
        if (!act)
            for (int i = 0; i < 6; i++) Jrow[i] = 0.;
        if (needJ) {
            int idx = 0;
            for (int a = 0; a < 6; a++) {
                for (int b = a; b < 6; b++) S[idx++] = grp_sum16(Jrow[a] * Jrow[b]);
                gJ[a] = grp_sum16(Jrow[a] * err);
            }
        }
    } while (lm.step(param, S, gJ, [&] { return grp_sum16(err * err); }, needJ));
    if (g == 0) {
        fid_stag_pose_out o;
        o.id = mk.id;
        for (int i = 0; i < 3; i++) {
            o.rvec[i] = param[i];
            o.tvec[i] = param[3 + i];
        }
        double dummy[27];
        rodrigues_v2m(param, o.R, dummy, false);  // cv::Rodrigues(rVec, rMat) of solvePnpSingle
        out[item] = o;
    }
    if constexpr (COV) {
        // ---- the covariance: J and e at the returned param, J^T J and |e|^2 over the marker's sixteen lanes
        const double pr = project_one<MODEL>(M, param, K, kd, sel, Jrow, true);
        const double ec = act ? pr - mobs : 0.;
        if (!act)
            for (int i = 0; i < 6; i++) Jrow[i] = 0.;
        int idx = 0;
        for (int a = 0; a < 6; a++)
            for (int b = a; b < 6; b++) S[idx++] = grp_sum16(Jrow[a] * Jrow[b]);
        const double e2 = grp_sum16(ec * ec);
        if (g == 0) pnp_covariance<false>(S, e2, 5, param, sigma_px, cov + item, nullptr);
    }
}
template <int MODEL>
__global__ __launch_bounds__(64) void k_stag_pose_cov(const fid_stag_marker *__restrict__ markers, const int *__restrict__ nmarkers, PoseCam cam, double marker_size, fid_stag_pose_out *__restrict__ out, double sigma_px, fid_pose_cov *__restrict__ cov)
{
    k_stag_pose_impl<MODEL, true>(markers, nmarkers, cam, marker_size, out, sigma_px, cov);
}
template <int MODEL>
struct k_stag_pose_fn {
    static constexpr int kBounds = 64;
    __device__ __forceinline__ void operator()(const fid_stag_marker *__restrict__ markers, const int *__restrict__ nmarkers, PoseCam cam, double marker_size, fid_stag_pose_out *__restrict__ out) const { k_stag_pose_impl<MODEL>(markers, nmarkers, cam, marker_size, out); }
};

// ------------------------------------------------------------------------------------------------ K18: bundle pose
// Common::solvePnpBundle (stag_ros/common.hpp:48-59): cv::solvePnP (ITERATIVE) over all points of all tags of a bundle that were
// seen -- per found tag its centre and c0..c3 (the layout's fid_stag_tag, bundle frame) against Marker::center / Marker::corners,
// the tags in the order their markers stand in the marker list.  One wave per bundle (blockIdx.x; the frames of a group ride in
// the trampoline's grid, fid_stag_batch.h):
//   (1) lanes scan the marker list for the bundle's ids (unique per frame after checkDuplicate) and gather the points into LDS;
//   (2) the planarity decision of cvFindExtrinsicCameraParams2: eigenvalues of the centred scatter matrix, w2 / w1 < 1e-3
//       (NOT the reference's checkCoplanar, common.hpp:85-103, which solvePnpBundle never calls);
//   (3) the start.  Coplanar: OpenCV's own -- the points turned into their plane by the scatter matrix's eigenvectors, the DLT
//       homography over ALL of them (HomographyEstimatorCallback::runKernel: float inputs, normalised, the 9 x 9 symmetric
//       eigenproblem by cyclic Jacobi in LDS, lane k the k-th row / column of a rotation), R and t from its columns.  Not coplanar
//       (tags on several faces): the closed-form four-corner pose of the found tag that is largest in the image, composed with that
//       tag's place in the bundle (OpenCV runs a 12 x 12 DLT there; parity unpinned);
//   (4) CvLevMarq (fid_pnp.h's LevMarq, as in k_stag_pose), the camera model's distortion (the template parameter) in the projection and its Jacobian.  Up to 120
//       residuals strided over the 64 lanes; J^T J (21), J^T e (6) and the norms are per-lane partial sums and one xor-butterfly
//       over the wave -- a fixed order: reproducible from run to run, the same value in every lane.
#define SB_MAX_TAGS 12  // FID_STAG_MAX_TAGS_PER_BUNDLE
#define SB_MAX_PTS (5 * SB_MAX_TAGS)
struct SbLds {
    double obj[SB_MAX_PTS][3], img[SB_MAX_PTS][2], mn[SB_MAX_PTS][2], Mxy[SB_MAX_PTS][2];
    double A[81], V[81], area[SB_MAX_TAGS];
    int ids[SB_MAX_TAGS], tagof[SB_MAX_TAGS], mk[SB_MAX_TAGS];
};

// HomographyEstimatorCallback::runKernel (fundam.cpp) over the n correspondences Mxy -> mn in LDS (both already rounded to
// float, as findHomography converts its inputs); every lane returns the same H
__device__ bool sb_homography_dlt(SbLds *s, int n, int lane, double H[9])
{
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    for (int i = 0; i < n; i++) {
        cmx += s->mn[i][0];
        cmy += s->mn[i][1];
        cMx += s->Mxy[i][0];
        cMy += s->Mxy[i][1];
    }
    cmx /= n; cmy /= n; cMx /= n; cMy /= n;
    for (int i = 0; i < n; i++) {
        smx += fabs(s->mn[i][0] - cmx);
        smy += fabs(s->mn[i][1] - cmy);
        sMx += fabs(s->Mxy[i][0] - cMx);
        sMy += fabs(s->Mxy[i][1] - cMy);
    }
    if (!(fabs(smx) >= DBL_EPSILON) || !(fabs(smy) >= DBL_EPSILON) || !(fabs(sMx) >= DBL_EPSILON) || !(fabs(sMy) >= DBL_EPSILON)) return false;
    smx = n / smx; smy = n / smy; sMx = n / sMx; sMy = n / sMy;
    // LtL: lane e < 45 owns entry (j, k), j <= k, and sums it over the points in their order
    if (lane < 45) {
        int j = 0, k = lane;
        while (k >= 9 - j) {
            k -= 9 - j;
            j++;
        }
        k += j;
        double acc = 0;
        for (int i = 0; i < n; i++) {
            const double x = (s->mn[i][0] - cmx) * smx, y = (s->mn[i][1] - cmy) * smy;
            const double X = (s->Mxy[i][0] - cMx) * sMx, Y = (s->Mxy[i][1] - cMy) * sMy;
            double lxj, lyj, lxk, lyk;
            pnp_dlt_entry(j, X, Y, x, y, &lxj, &lyj);
            pnp_dlt_entry(k, X, Y, x, y, &lxk, &lyk);
            acc += lxj * lxk + lyj * lyk;
        }
        s->A[j * 9 + k] = acc;
        s->A[k * 9 + j] = acc;
    }
    return pnp_dlt_finish(s->A, s->V, lane, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
}

// COV: the covariance tail (fid_abi.h: "pose covariance"; k_stag_bundle_pose_cov) over the same points, with this kernel's wave sum
template <int MODEL, bool COV = false>
__device__ __forceinline__ void k_stag_bundle_pose_impl(const fid_stag_marker *__restrict__ markers, const int *__restrict__ nmarkers,
                                                         const fid_stag_tag *__restrict__ ltags, const int *__restrict__ lstart, PoseCam cam,
                                                         fid_stag_bundle_pose_out *__restrict__ out, double sigma_px = 0.,
                                                         fid_pose_cov *__restrict__ cov = nullptr)
{
    __shared__ SbLds s;
    const int b = blockIdx.x, lane = threadIdx.x;
    const double *K = cam.K, *kd = cam.D;
    const int t0 = lstart[b];
    int nt = lstart[b + 1] - t0;
    nt = nt < 0 ? 0 : (nt > SB_MAX_TAGS ? SB_MAX_TAGS : nt);
    const int nm = *nmarkers;
    // ---- (1) the bundle's tags among the frame's markers, in marker order
    if (lane < nt) s.ids[lane] = ltags[t0 + lane].id;
    SR_LDS_SYNC();
    int found = 0;
    for (int m0 = 0; m0 < nm && found < SB_MAX_TAGS; m0 += 64) {
        const int m = m0 + lane;
        int ti = -1;
        if (m < nm) {
            const int id = markers[m].id;
            for (int k = nt - 1; k >= 0; k--)
                if (s.ids[k] == id) ti = k;
        }
        const unsigned long long hit = __ballot(ti >= 0);
        if (ti >= 0) {
            const int pos = found + __builtin_popcountll(hit & ((1ull << lane) - 1ull));
            if (pos < SB_MAX_TAGS) {
                s.tagof[pos] = ti;
                s.mk[pos] = m;
            }
        }
        found += __builtin_popcountll(hit);
    }
    found = found > SB_MAX_TAGS ? SB_MAX_TAGS : found;
    if (found == 0) {
        if (lane == 0) {
            fid_stag_bundle_pose_out o;
            o.bundle = b;
            o.n_tags = 0;
            for (int i = 0; i < 3; i++) o.rvec[i] = o.tvec[i] = 0.;
            for (int i = 0; i < 9; i++) o.R[i] = 0.;
            out[b] = o;
            if constexpr (COV) pnp_cov_zero(cov + b, 1, 0, nullptr);
        }
        return;
    }
    SR_LDS_SYNC();
    const int npts = 5 * found;
    bool posable = true;
    if (lane < npts) {
        const int p = lane / 5, q = lane % 5;
        const fid_stag_tag *tg = ltags + t0 + s.tagof[p];
        const fid_stag_marker *mk = markers + s.mk[p];
        for (int a = 0; a < 3; a++) s.obj[lane][a] = q == 0 ? tg->center[a] : tg->corners[q - 1][a];
        const double u = q == 0 ? mk->center[0] : mk->corners[2 * (q - 1)], v = q == 0 ? mk->center[1] : mk->corners[2 * (q - 1) + 1];
        s.img[lane][0] = u;
        s.img[lane][1] = v;
        double x, y;
        const bool ok = pnp_undistort<MODEL>(K, kd, u, v, &x, &y);
        if constexpr (MODEL == FID_CAM_EQUIDISTANT) posable = ok;
        s.mn[lane][0] = (double)(float)x;  // (the DLT's input: findHomography converts to float)
        s.mn[lane][1] = (double)(float)y;
        if (q == 0) {  // the tag's area in the image (shoelace over its four corners)
            double a2 = 0;
            for (int i = 0; i < 4; i++) {
                const int i1 = (i + 1) & 3;
                a2 += mk->corners[2 * i] * mk->corners[2 * i1 + 1] - mk->corners[2 * i1] * mk->corners[2 * i + 1];
            }
            s.area[p] = fabs(a2);
        }
    }
    SR_LDS_SYNC();
    if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
        if (__ballot(!posable) != 0ull) {  // a point beyond the model (fid_abi.h: "a marker that cannot be posed") voids the bundle's record
            if (lane == 0) {
                fid_stag_bundle_pose_out o;
                o.bundle = b;
                o.n_tags = found;
                for (int i = 0; i < 3; i++) o.rvec[i] = o.tvec[i] = 0.;
                for (int i = 0; i < 9; i++) o.R[i] = 0.;
                out[b] = o;
                if constexpr (COV) pnp_cov_zero(cov + b, 1, npts, nullptr);
            }
            return;
        }
    }
    // ---- (2) planarity: the centred scatter matrix of the object points and its eigenvalues (every lane the same)
    double Mc[3] = {0, 0, 0}, W[3], Vt[3][3];
    {
        double MM[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int i = 0; i < npts; i++)
            for (int a = 0; a < 3; a++) Mc[a] += s.obj[i][a];
        for (int a = 0; a < 3; a++) Mc[a] /= npts;
        for (int i = 0; i < npts; i++) {
            const double d[3] = {s.obj[i][0] - Mc[0], s.obj[i][1] - Mc[1], s.obj[i][2] - Mc[2]};
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int c = 0; c < 3; c++) MM[a][c] += d[a] * d[c];
        }
        pnp_scatter_eig(MM, W, Vt);
    }
    const bool planar = W[2] / W[1] < 1e-3;
    // ---- (3) the start
    double param[6] = {0, 0, 0, 0, 0, 0};
    if (planar) {
        double Rt[9], tt[3];
        pnp_plane_frame(Vt, Mc, Rt, tt);
        if (lane < npts) {
            const double *src = s.obj[lane];
            s.Mxy[lane][0] = (double)(float)(Rt[0] * src[0] + Rt[1] * src[1] + Rt[2] * src[2] + tt[0]);
            s.Mxy[lane][1] = (double)(float)(Rt[3] * src[0] + Rt[4] * src[1] + Rt[5] * src[2] + tt[1]);
        }
        SR_LDS_SYNC();
        double h[9], R[9];
        if (sb_homography_dlt(&s, npts, lane, h)) {
            double t3[3];
            pnp_pose_from_h(h, t3);
            for (int i = 0; i < 3; i++) param[3 + i] = h[i * 3] * tt[0] + h[i * 3 + 1] * tt[1] + h[i * 3 + 2] * tt[2] + t3[i];
            pnp_mul3(h, Rt, R);
        } else {
            for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1. : 0.;
        }
        rodrigues_m2v(R, param);
    } else {
        int big = 0;
        for (int p = 1; p < found; p++)
            if (s.area[p] > s.area[big]) big = p;
        // (a tag's points: its centre, then c0..c3)
        pnp_start_largest<MODEL>(s.obj[5 * big + 1], s.obj[5 * big + 2], s.obj[5 * big + 4], s.obj[5 * big], s.img + 5 * big + 1, K, kd, param);
    }
    // ---- (4) CvLevMarq over the 2 * npts residuals: lane l owns residuals l and l + 64
    const int nres = 2 * npts;
    const bool act0 = lane < nres, act1 = lane + 64 < nres;
    const int r0 = act0 ? lane : 0, r1 = act1 ? lane + 64 : 0;
    const double M0[3] = {s.obj[r0 >> 1][0], s.obj[r0 >> 1][1], s.obj[r0 >> 1][2]}, M1[3] = {s.obj[r1 >> 1][0], s.obj[r1 >> 1][1], s.obj[r1 >> 1][2]};
    const double mobs0 = s.img[r0 >> 1][r0 & 1], mobs1 = s.img[r1 >> 1][r1 & 1];
    double S[21], gJ[6], J0[6] = {0, 0, 0, 0, 0, 0}, J1[6] = {0, 0, 0, 0, 0, 0}, err0 = 0, err1 = 0;
    bool needJ = true;
    LevMarq lm;
    do {
        if (act0) {
            err0 = project_one<MODEL>(M0, param, K, kd, r0 & 1, J0, needJ) - mobs0;
        } else {
            err0 = 0.;
            for (int i = 0; i < 6; i++) J0[i] = 0.;
        }
        if (act1) {
            err1 = project_one<MODEL>(M1, param, K, kd, r1 & 1, J1, needJ) - mobs1;
        } else {
            err1 = 0.;
            for (int i = 0; i < 6; i++) J1[i] = 0.;
        }
        if (needJ) {
            int idx = 0;
            for (int a = 0; a < 6; a++) {
                for (int c = a; c < 6; c++) S[idx++] = wave_sum_f64(J0[a] * J0[c] + J1[a] * J1[c]);
                gJ[a] = wave_sum_f64(J0[a] * err0 + J1[a] * err1);
            }
        }
    } while (lm.step(param, S, gJ, [&] { return wave_sum_f64(err0 * err0 + err1 * err1); }, needJ));
    if (lane == 0) {
        fid_stag_bundle_pose_out o;
        o.bundle = b;
        o.n_tags = found;
        for (int i = 0; i < 3; i++) {
            o.rvec[i] = param[i];
            o.tvec[i] = param[3 + i];
        }
        double dummy[27];
        rodrigues_v2m(param, o.R, dummy, false);
        out[b] = o;
    }
    if constexpr (COV) {
        // ---- the covariance: J and e at the returned param, J^T J and |e|^2 over the wave (two residuals per lane)
        if (act0) {
            err0 = project_one<MODEL>(M0, param, K, kd, r0 & 1, J0, true) - mobs0;
        } else {
            err0 = 0.;
            for (int i = 0; i < 6; i++) J0[i] = 0.;
        }
        if (act1) {
            err1 = project_one<MODEL>(M1, param, K, kd, r1 & 1, J1, true) - mobs1;
        } else {
            err1 = 0.;
            for (int i = 0; i < 6; i++) J1[i] = 0.;
        }
        int idx = 0;
        for (int a = 0; a < 6; a++)
            for (int c = a; c < 6; c++) S[idx++] = wave_sum_f64(J0[a] * J0[c] + J1[a] * J1[c]);
        const double e2 = wave_sum_f64(err0 * err0 + err1 * err1);
        if (lane == 0) pnp_covariance<false>(S, e2, npts, param, sigma_px, cov + b, nullptr);
    }
}
template <int MODEL>
__global__ __launch_bounds__(64) void k_stag_bundle_pose_cov(const fid_stag_marker *__restrict__ markers, const int *__restrict__ nmarkers, const fid_stag_tag *__restrict__ ltags, const int *__restrict__ lstart, PoseCam cam, fid_stag_bundle_pose_out *__restrict__ out, double sigma_px, fid_pose_cov *__restrict__ cov)
{
    k_stag_bundle_pose_impl<MODEL, true>(markers, nmarkers, ltags, lstart, cam, out, sigma_px, cov);
}
template <int MODEL>
struct k_stag_bundle_pose_fn {
    static constexpr int kBounds = 64;
    __device__ __forceinline__ void operator()(const fid_stag_marker *__restrict__ markers, const int *__restrict__ nmarkers, const fid_stag_tag *__restrict__ ltags, const int *__restrict__ lstart, PoseCam cam, fid_stag_bundle_pose_out *__restrict__ out) const { k_stag_bundle_pose_impl<MODEL>(markers, nmarkers, ltags, lstart, cam, out); }
};
