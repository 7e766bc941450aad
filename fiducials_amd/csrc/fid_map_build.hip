// fid_map_build.hip -- the map from a set of views by bundle adjustment (fid_abi.h: "building the map").  Part of the fid_api.hip
// translation unit.  The residual function (cal_rotation_value, cal_pinhole, cal_distort, cal_project, cal_row,
// cal_rotation_lds) is the calibration's, fid_cal_model.h; k_pose and k_map_pose give the start; solve6_spd and the damping table come from fid_pnp.h.
//
// With a 6 x 6 block per marker (A_i) and per view (C_v) the normal matrix is bipartite: the couplings B_vi (6 x 6, marker rows, view
// columns) exist where view v holds marker i.  Eliminating the views leaves the reduced system over the free markers,
//     S_ij = [i == j] sum_v A_vi (1 + lambda on its diagonal) - sum_v W_vi B_vj^T,   W_vi = B_vi (C_v + lambda diag C_v)^-1,
//     s_i  = sum_v a_vi - sum_v W_vi g_v,
// n = 6 x (free markers) <= 762 rows (at least one of the 128 markers is fixed).  One trial step of Levenberg-Marquardt, all on the
// context's stream:
//   k_build_prep     a wave per marker, after an accepted step: R and dR / d rvec of its pose (cal_rotation_lds).
//   k_build_blocks   a wave per view.  After an accepted step: the view's residual rows, 64 at a time = 8 observations -- a lane makes
//                    one row of 13 (6 marker columns, 6 view columns, the residual) in LDS; then lane w adds ITS entry of each
//                    observation's 64 (A 21, B 36, a 6, e.e) over the observation's 8 rows, and lanes 0 .. 26 theirs of C_v and g_v
//                    over all rows: each entry one serial sum in row order.
//   k_build_schur    a wave per view, every trial: W_vi and W_vi g_v under the current damping (solve6_spd, a lane per row).
//   k_build_reduce   a wave per 6 x 6 block (i, j), j <= i: lane (a, b) walks the views that hold both markers -- two ascending lists --
//                    in view order.
//   k_build_panel /  the Cholesky factor, right-looking in panels of 32 columns, two launches per panel: every workgroup factors the
//   k_build_update   32 x 32 diagonal block in LDS for itself (the same arithmetic, so the same bytes) and solves its 32 rows of the
//                    panel; then a workgroup per 32 x 32 tile of the trailing matrix subtracts the panel's product, each entry one
//                    serial sum over the 32 columns.  The order of every sum is the code's; no workgroup waits for another, and
//                    no launch writes what another workgroup of it reads (the factored diagonal blocks go to a side array).
//   k_build_solve    one workgroup: the two triangular solves in blocks of 32 through LDS, the markers' candidates, the current cost.
//   k_build_eval     a wave per view: its step by back-substitution, the candidate pose, the cost there.
//   k_build_accept   one workgroup: the candidate's cost, accept / reject, the stop.
// Every kernel of a trial returns at once when the stop has been reached, so the host queues BLD_CHUNK trials between two reads of the
// 16-byte status.  After the stop, undamped: prep, blocks, schur, k_build_finish (the records), reduce, the factor, and k_build_cov -- a
// workgroup per marker solves L z = e for the marker's six unit columns; the block of the inverse is z^T z.
// No kernel keeps a run-time indexed array in registers; no scratch, no spills (tests/test_map_build_kernel_allocations.py).
// fid_build_map_robust_cam (the trimmed build) runs the same trial kernels in rounds, behind a start and between error passes of its
// own: k_build_place_score and k_build_obs_err, in front of the host section below.

#include "fid_cal_model.h"

#define BLD_NB 32
#define BLD_OB 64   // doubles of an observation's record: A (21, upper triangle) | B (36, marker row x view column) | a (6) | e.e
#define BLD_OW 42   // W_vi (36) | W_vi g_v (6)
#define BLD_VB 27   // C_v (21) | g_v (6)
#define BLD_MR 48   // a marker's rotation record: R (9) | dR / d rvec (27) | t (3) | h | unused
#ifndef BLD_CHUNK
#define BLD_CHUNK 8
#endif

struct BldCfg {
    int n_views, n_slots, n_fm, n;  // views, markers in the solve, free markers, 6 n_fm
    int per_view, max_iter, n_obs, n_points;
    int n_views_used, n_free, pad0, pad1;
    double eps, sigma_px;
};
struct BldState {
    double cost, start_cost, dnM, pnM, ctot;
    int lambdaLg10, trials, status, done;  // (read back together)
    int needJ, bad, pad0, pad1;
};

// the sum of one value per thread of a 256-thread workgroup in a fixed tree; every thread gets it
__device__ __forceinline__ double bld_sum256(double v, double *buf, int t)
{
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    return buf[0];
}

// (a, b), a <= b, of entry w of the packed upper triangle of a 6 x 6 matrix (solve6_spd's order)
__device__ __forceinline__ void bld_untri6(int w, int *a, int *b)
{
    int i = 0, r = w;
    while (r >= 6 - i) {
        r -= 6 - i;
        i++;
    }
    *a = i;
    *b = i + r;
}

// ------------------------------------------------------------------------------------------------ the markers' rotations
__global__ WALKER_WG_ATTR(64, 1024) void k_build_prep(const BldState *__restrict__ st, const int *__restrict__ mfree, const double *__restrict__ mpar,
                                                    double *__restrict__ mrt, int final)
{
    __shared__ double rot[36], rtmp[80];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (!final && (st->done || !st->needJ)) return;
    if (mfree[s] < 0) return;  // (a fixed marker's record is the host's)
    cal_rotation_lds(mpar + 6 * s, rot, rtmp, lane);
    if (lane < 36) mrt[BLD_MR * s + lane] = rot[lane];
    if (lane < 3) mrt[BLD_MR * s + 36 + lane] = mpar[6 * s + 3 + lane];
}

// ------------------------------------------------------------------------------------------------ a view's blocks
// voff / vcnt: the view's observations [voff, voff + vcnt) (vcnt = 0: a skipped view); omk: the observation's marker in the list,
// oslot: its slot; mfree[slot]: its index among the free markers, or -1.
template <int MODEL>
__global__ WALKER_WG_ATTR(64, 1024) void k_build_blocks(const BldState *__restrict__ st, PoseCam cam, const fid_marker *__restrict__ markers,
                                                      const int *__restrict__ voff, const int *__restrict__ vcnt, const int *__restrict__ omk,
                                                      const int *__restrict__ oslot, const int *__restrict__ mfree, const double *__restrict__ mrt,
                                                      const double *__restrict__ vpose, double *__restrict__ oblk, double *__restrict__ vblk,
                                                      double *__restrict__ vcost, int final)
{
    __shared__ double rows[64][13];
    __shared__ double rot[36], rtmp[80];
    const int v = blockIdx.x, lane = threadIdx.x;
    if (!final && st->done) return;
    const int cnt = vcnt[v], off = voff[v];
    if (cnt <= 0) return;
    if (!final && !st->needJ) return;  // (a rejected trial: the blocks stand)
    {
        cal_rotation_lds(vpose + 6 * v, rot, rtmp, lane);
        // this lane's entry of the view's 27 and of an observation's 64: the two columns of a row it multiplies
        int ca = 6, cb = 6, pa, pb;
        if (lane < 21) {
            bld_untri6(lane, &ca, &cb);
            ca += 6;
            cb += 6;
        } else if (lane < BLD_VB) {
            ca = 6 + (lane - 21);
            cb = 12;
        }
        if (lane < 21) {
            bld_untri6(lane, &pa, &pb);
        } else if (lane < 57) {
            pa = (lane - 21) / 6;
            pb = 6 + (lane - 21) % 6;
        } else if (lane < 63) {
            pa = lane - 57;
            pb = 12;
        } else {
            pa = pb = 12;
        }
        double tv[3];
#pragma unroll
        for (int i = 0; i < 3; i++) tv[i] = vpose[6 * v + 3 + i];
        const int nres = 8 * cnt;
        double accv = 0., e2 = 0.;
        for (int r0 = 0; r0 < nres; r0 += 64) {
            const int r = r0 + lane;
            if (r < nres) {
                const int k = r >> 3, q = (r >> 1) & 3, su = r & 1, o = off + k;
                const int slot = oslot[o];
                const double *mr = mrt + (size_t)BLD_MR * slot;
                const double h = mr[39];
                const double X = (q == 0 || q == 3) ? -h : h, Y = q < 2 ? h : -h;
                double P[3];
#pragma unroll
                for (int a = 0; a < 3; a++) P[a] = mr[3 * a] * X + mr[3 * a + 1] * Y + mr[36 + a];
                double *row = rows[lane];
                int roff = 0;
                asm volatile("" : "+v"(roff));  // (as k_calib_blocks: the rotation is read from LDS where it is used)
                double dI[16];  // (never read: the intrinsics' derivatives fall away)
                // (cal_row stores the view's six columns into the row as it has them: no lane holds them at once)
                const double err = cal_row<MODEL>(P, rot + roff, rot + roff + 9, tv, cam.K, cam.D, su, row + 6, dI) - (double)markers[omk[o]].corners[2 * q + su];
                row[12] = err;
                e2 += err * err;
                if (mfree[slot] >= 0) {
                    // d / d p_map = (d / d p_cam) R_v; through the marker's pose: d p_map / d t = I, d p_map / d rvec_j = dR_j M
                    // (the marker's derivative is read only now: an offset that waits for the residual keeps its 18 loads from being
                    // hoisted above cal_row into registers of every lane)
                    int moff2 = 0;
                    asm volatile("" : "+v"(moff2) : "v"(err));
                    const double *Rv = rot + roff, *md = mr + moff2;
                    const double w0 = row[9], w1 = row[10], w2 = row[11];  // d / d p_cam = d / d tvec
                    double u[3];
#pragma unroll
                    for (int j = 0; j < 3; j++) u[j] = w0 * Rv[j] + w1 * Rv[3 + j] + w2 * Rv[6 + j];
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const double *d9 = md + 9 + 9 * j;
                        row[j] = u[0] * (d9[0] * X + d9[1] * Y) + u[1] * (d9[3] * X + d9[4] * Y) + u[2] * (d9[6] * X + d9[7] * Y);
                        row[3 + j] = u[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 6; j++) row[j] = 0.;
                }
            }
            SR_LDS_SYNC();
            const int cntr = nres - r0 < 64 ? nres - r0 : 64;
#pragma unroll 4
            for (int i = 0; i < cntr; i++) accv += rows[i][ca] * rows[i][cb];
            const int nob = cntr >> 3;
            for (int k = 0; k < nob; k++) {
                double s = 0.;
#pragma unroll
                for (int i = 0; i < 8; i++) s += rows[8 * k + i][pa] * rows[8 * k + i][pb];
                oblk[(size_t)(off + (r0 >> 3) + k) * BLD_OB + lane] = s;
            }
            SR_LDS_SYNC();
        }
        if (lane < BLD_VB) vblk[(size_t)v * BLD_VB + lane] = accv;
        e2 = wave_sum_f64(e2);
        if (lane == 0) vcost[v] = e2;
    }
}

// W_vi = B_vi (C_v + lambda diag C_v)^-1 and W_vi g_v under the current damping: a wave per view, row a of observation k by one lane
__global__ WALKER_WG_ATTR(64, 1024) void k_build_schur(const BldState *__restrict__ st, const int *__restrict__ voff, const int *__restrict__ vcnt,
                                                     const int *__restrict__ oslot, const int *__restrict__ mfree, const double *__restrict__ oblk,
                                                     const double *__restrict__ vblk, double *__restrict__ ow, int final)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    if (!final && st->done) return;
    const int cnt = vcnt[v], off = voff[v];
    if (cnt <= 0) return;
    const double lambda = final ? 0. : lm_lambda(st->lambdaLg10);
    double S[21], gP[6];
#pragma unroll
    for (int i = 0; i < 21; i++) S[i] = vblk[(size_t)v * BLD_VB + i];
#pragma unroll
    for (int i = 0; i < 6; i++) gP[i] = vblk[(size_t)v * BLD_VB + 21 + i];
    for (int it = lane; it < 6 * cnt; it += 64) {
        const int k = it / 6, a = it - 6 * k, o = off + k;
        if (mfree[oslot[o]] < 0) continue;
        double Bj[6], Wj[6];
#pragma unroll
        for (int b = 0; b < 6; b++) Bj[b] = oblk[(size_t)o * BLD_OB + 21 + 6 * a + b];
        solve6_spd(S, Bj, lambda, Wj);
        double rj = 0.;
#pragma unroll
        for (int b = 0; b < 6; b++) {
            ow[(size_t)o * BLD_OW + 6 * a + b] = Wj[b];
            rj += Wj[b] * gP[b];
        }
        ow[(size_t)o * BLD_OW + 36 + a] = rj;
    }
}

// ------------------------------------------------------------------------------------------------ the reduced system
// grid (n_fm, n_fm): block (i, j) of the lower triangle.  fslot: the slot of free marker i; moff / mobs: the slot's observations in view
// order; oview: an observation's view.  Sm: n x n row-major, the lower triangle is written; g: the right-hand side.
__global__ __launch_bounds__(64) void k_build_reduce(const BldCfg *__restrict__ cfg, BldState *__restrict__ st, const int *__restrict__ fslot,
                                                      const int *__restrict__ moff, const int *__restrict__ mobs, const int *__restrict__ oview,
                                                      const double *__restrict__ oblk, const double *__restrict__ ow, double *__restrict__ Sm,
                                                      double *__restrict__ g, int final)
{
    const int i = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    if (j > i) return;
    if (!final && st->done) return;
    if (i == 0 && lane == 0) st->bad = 0;
    const int n = cfg->n;
    const double lambda = final ? 0. : lm_lambda(st->lambdaLg10);
    const bool diag = i == j, mat = lane < 36, rhs = diag && lane >= 36 && lane < 42;
    if (!mat && !rhs) return;
    const int a = mat ? lane / 6 : lane - 36, b = mat ? lane - 6 * a : 0;
    int ta = a < b ? a : b, tb = a < b ? b : a;
    const int te = ta * 6 - ta * (ta - 1) / 2 + (tb - ta);  // A's entry (a, b) in its packed triangle
    const int si = fslot[i], sj = fslot[j];
    int p = moff[si], q = moff[sj];
    const int pe = moff[si + 1], qe = moff[sj + 1];
    double sA = 0., sS = 0.;
    while (p < pe && q < qe) {
        const int oi = mobs[p], oj = mobs[q];
        const int vi = oview[oi], vj = oview[oj];
        if (vi < vj) {
            p++;
        } else if (vj < vi) {
            q++;
        } else {
            if (mat) {
                const double *w = ow + (size_t)oi * BLD_OW + 6 * a, *bj = oblk + (size_t)oj * BLD_OB + 21 + 6 * b;
                double s = 0.;
#pragma unroll
                for (int c = 0; c < 6; c++) s += w[c] * bj[c];
                sS += s;
                if (diag) sA += oblk[(size_t)oi * BLD_OB + te];
            } else {
                sS += ow[(size_t)oi * BLD_OW + 36 + a];
                sA += oblk[(size_t)oi * BLD_OB + 57 + a];
            }
            p++;
            q++;
        }
    }
    if (mat)
        Sm[(size_t)(6 * i + a) * n + 6 * j + b] = (diag && a == b ? sA * (1. + lambda) : sA) - sS;
    else
        g[6 * i + a] = sA - sS;
}

// ------------------------------------------------------------------------------------------------ the Cholesky factor, a panel step
// the 32 x 32 diagonal block at k0 into LDS, factored in place (a lane per row); false: no factor
__device__ __forceinline__ bool bld_factor_diag(const double *__restrict__ Sm, int n, int k0, int nb, double (*D)[BLD_NB + 1], int lane)
{
    for (int e = lane; e < nb * nb; e += 64) {
        const int r = e / nb, c = e - r * nb;
        if (c <= r) D[r][c] = Sm[(size_t)(k0 + r) * n + k0 + c];
    }
    SR_LDS_SYNC();
    for (int j = 0; j < nb; j++) {
        const double dj = D[j][j];
        if (!(dj > 0.) || !(dj - dj == 0.)) return false;  // (every lane reads the same value)
        const double sq = sqrt(dj);
        SR_LDS_SYNC();
        if (lane == j) D[j][j] = sq;
        if (lane > j && lane < nb) D[lane][j] = D[lane][j] / sq;
        SR_LDS_SYNC();
        if (lane > j && lane < nb)
            for (int k = j + 1; k <= lane; k++) D[lane][k] -= D[lane][j] * D[k][j];
        SR_LDS_SYNC();
    }
    return true;
}

// grid ceil((n - k0) / 32): workgroup t >= 1 solves rows k0 + 32 t .. of the panel; workgroup 0 stores the factored diagonal block in
// Dg (block k0 / 32, 32 x 32 row-major), NOT back into Sm: every workgroup of this launch reads the unfactored block from Sm, so the
// launch never writes it -- whichever workgroup starts when, it factors the same bytes.  k_build_solve and k_build_cov take the
// factored diagonal blocks from Dg and the rows below them from Sm.
__global__ WALKER_WG_ATTR(64, 1024) void k_build_panel(const BldCfg *__restrict__ cfg, BldState *__restrict__ st, double *__restrict__ Sm, double *__restrict__ Dg, int k0, int final)
{
    __shared__ double D[BLD_NB][BLD_NB + 1], P[BLD_NB][BLD_NB + 1];
    const int tile = blockIdx.x, lane = threadIdx.x;
    if (!final && st->done) return;
    const int n = cfg->n;
    if (k0 >= n) return;
    const int nb = n - k0 < BLD_NB ? n - k0 : BLD_NB;
    if (!bld_factor_diag(Sm, n, k0, nb, D, lane)) {
        if (tile == 0 && lane == 0) st->bad = 1;
        return;
    }
    if (tile == 0) {
        for (int e = lane; e < nb * nb; e += 64) {
            const int r = e / nb, c = e - r * nb;
            if (c <= r) Dg[(size_t)(k0 / BLD_NB) * BLD_NB * BLD_NB + r * BLD_NB + c] = D[r][c];
        }
        return;
    }
    const int rb = k0 + BLD_NB * tile;
    if (rb >= n) return;
    const int nr = n - rb < BLD_NB ? n - rb : BLD_NB;
    for (int e = lane; e < nr * BLD_NB; e += 64) {
        const int r = e / BLD_NB, c = e - r * BLD_NB;
        P[r][c] = Sm[(size_t)(rb + r) * n + k0 + c];
    }
    SR_LDS_SYNC();
    if (lane < nr) {  // x L^T = the row: column j after the columns before it
        for (int j = 0; j < BLD_NB; j++) {
            double s = P[lane][j];
            for (int k = 0; k < j; k++) s -= P[lane][k] * D[j][k];
            P[lane][j] = s / D[j][j];
        }
    }
    SR_LDS_SYNC();
    for (int e = lane; e < nr * BLD_NB; e += 64) {
        const int r = e / BLD_NB, c = e - r * BLD_NB;
        Sm[(size_t)(rb + r) * n + k0 + c] = P[r][c];
    }
}

// grid (T, T), T = ceil((n - k0 - 32) / 32): tile (ti, tj), tj <= ti, of the trailing matrix minus the panel's product
__global__ __launch_bounds__(256) void k_build_update(const BldCfg *__restrict__ cfg, const BldState *__restrict__ st, double *__restrict__ Sm, int k0, int final)
{
    __shared__ double Lr[BLD_NB][BLD_NB + 1], Lc[BLD_NB][BLD_NB + 1];
    const int ti = blockIdx.x, tj = blockIdx.y, t = threadIdx.x;
    if (tj > ti) return;
    if (!final && st->done) return;
    const int n = cfg->n, base = k0 + BLD_NB;
    const int ri = base + BLD_NB * ti, rj = base + BLD_NB * tj;
    if (ri >= n) return;
    const int ni = n - ri < BLD_NB ? n - ri : BLD_NB, nj = n - rj < BLD_NB ? n - rj : BLD_NB;
    for (int e = t; e < BLD_NB * BLD_NB; e += 256) {
        const int r = e >> 5, c = e & 31;
        Lr[r][c] = r < ni ? Sm[(size_t)(ri + r) * n + k0 + c] : 0.;
        Lc[r][c] = r < nj ? Sm[(size_t)(rj + r) * n + k0 + c] : 0.;
    }
    __syncthreads();
    const int r = t >> 3, c0 = (t & 7) * 4;
    if (r >= ni) return;
    for (int cc = 0; cc < 4; cc++) {
        const int c = c0 + cc;
        if (c >= nj) break;
        double s = Sm[(size_t)(ri + r) * n + rj + c];
        for (int p = 0; p < BLD_NB; p++) s -= Lr[r][p] * Lc[c][p];
        Sm[(size_t)(ri + r) * n + rj + c] = s;
    }
}

// ------------------------------------------------------------------------------------------------ the step, the markers' candidates
__global__ __launch_bounds__(256) void k_build_solve(const BldCfg *__restrict__ cfg, BldState *__restrict__ st, const double *__restrict__ Sm, const double *__restrict__ Dg,
                                                      const double *__restrict__ g, const int *__restrict__ mfree, const double *__restrict__ mpar,
                                                      const int *__restrict__ vcnt, const double *__restrict__ vcost, double *__restrict__ dx,
                                                      double *__restrict__ mcand, double *__restrict__ crt)
{
    __shared__ double x[6 * FID_BUILD_MAX_MARKERS], D[BLD_NB][BLD_NB + 1], buf[256];
    const int t = threadIdx.x;
    if (st->done) return;
    const int n = cfg->n, nv = cfg->n_views;
    const bool bad = st->bad != 0;
    for (int i = t; i < n; i += 256) x[i] = bad ? 0. : g[i];
    __syncthreads();
    if (!bad) {
        // ---- L y = s, blocks of 32 rows from the top
        for (int k0 = 0; k0 < n; k0 += BLD_NB) {
            const int nb = n - k0 < BLD_NB ? n - k0 : BLD_NB;
            for (int e = t; e < nb * nb; e += 256) {
                const int r = e / nb, c = e - r * nb;
                if (c <= r) D[r][c] = Dg[(size_t)(k0 / BLD_NB) * BLD_NB * BLD_NB + r * BLD_NB + c];
            }
            __syncthreads();
            if (t < 64) {
                for (int j = 0; j < nb; j++) {
                    if (t == 0) x[k0 + j] = x[k0 + j] / D[j][j];
                    SR_LDS_SYNC();
                    if (t > j && t < nb) x[k0 + t] -= D[t][j] * x[k0 + j];
                    SR_LDS_SYNC();
                }
            }
            __syncthreads();
            for (int r = k0 + nb + t; r < n; r += 256) {
                double s = x[r];
                for (int p = 0; p < nb; p++) s -= Sm[(size_t)r * n + k0 + p] * x[k0 + p];
                x[r] = s;
            }
            __syncthreads();
        }
        // ---- L^T x = y, from the bottom
        for (int k0 = ((n - 1) / BLD_NB) * BLD_NB; k0 >= 0; k0 -= BLD_NB) {
            const int nb = n - k0 < BLD_NB ? n - k0 : BLD_NB;
            for (int e = t; e < nb * nb; e += 256) {
                const int r = e / nb, c = e - r * nb;
                if (c <= r) D[r][c] = Dg[(size_t)(k0 / BLD_NB) * BLD_NB * BLD_NB + r * BLD_NB + c];
            }
            __syncthreads();
            if (t < 64) {
                for (int j = nb - 1; j >= 0; j--) {
                    if (t == 0) x[k0 + j] = x[k0 + j] / D[j][j];
                    SR_LDS_SYNC();
                    if (t < j) x[k0 + t] -= D[j][t] * x[k0 + j];
                    SR_LDS_SYNC();
                }
            }
            __syncthreads();
            for (int r = t; r < k0; r += 256) {
                double s = x[r];
                for (int p = 0; p < nb; p++) s -= Sm[(size_t)(k0 + p) * n + r] * x[k0 + p];
                x[r] = s;
            }
            __syncthreads();
        }
    }
    for (int i = t; i < n; i += 256) dx[i] = x[i];
    // ---- the markers' candidates, |step|^2 and |p|^2 of their parameters
    double dn = 0., pn = 0.;
    if (t < cfg->n_slots) {
        const int fi = mfree[t];
        if (fi >= 0) {
            double cp[6], R[9];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const double p0 = mpar[6 * t + a], d = x[6 * fi + a];
                cp[a] = p0 - d;
                dn += d * d;
                pn += p0 * p0;
                mcand[6 * t + a] = cp[a];
            }
            cal_rotation_value(cp, R);
#pragma unroll
            for (int k = 0; k < 9; k++) crt[12 * t + k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) crt[12 * t + 9 + k] = cp[3 + k];
        }
    }
    dn = bld_sum256(dn, buf, t);
    pn = bld_sum256(pn, buf, t);
    // ---- the cost at the current parameters (k_build_blocks has just written it)
    double cs = 0.;
    for (int v = t; v < nv; v += 256)
        if (vcnt[v] > 0) cs += vcost[v];
    cs = bld_sum256(cs, buf, t);
    if (t == 0) {
        st->dnM = dn;
        st->pnM = pn;
        if (st->needJ) {
            st->cost = cs;
            if (st->trials == 0) st->start_cost = cs;
        }
    }
}

// ------------------------------------------------------------------------------------------------ a view's candidate
template <int MODEL>
__global__ __launch_bounds__(64) void k_build_eval(const BldState *__restrict__ st, PoseCam cam, const fid_marker *__restrict__ markers,
                                                    const int *__restrict__ voff, const int *__restrict__ vcnt, const int *__restrict__ omk,
                                                    const int *__restrict__ oslot, const int *__restrict__ mfree, const double *__restrict__ mrt,
                                                    const double *__restrict__ crt, const double *__restrict__ vpose, const double *__restrict__ oblk,
                                                    const double *__restrict__ vblk, const double *__restrict__ dx, double *__restrict__ vcand,
                                                    double *__restrict__ vccost, double *__restrict__ dnpn)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    if (st->done || st->bad) return;
    const int cnt = vcnt[v], off = voff[v];
    if (cnt <= 0) return;
    double S[21], rhs[6], param[6], dP[6];
#pragma unroll
    for (int i = 0; i < 21; i++) S[i] = vblk[(size_t)v * BLD_VB + i];
#pragma unroll
    for (int i = 0; i < 6; i++) rhs[i] = vblk[(size_t)v * BLD_VB + 21 + i];
    for (int k = 0; k < cnt; k++) {  // g_v - sum_i B_vi^T x_i, the observations in list order
        const int o = off + k, fi = mfree[oslot[o]];
        if (fi < 0) continue;
        const double *B = oblk + (size_t)o * BLD_OB + 21;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double da = dx[6 * fi + a];
#pragma unroll
            for (int b = 0; b < 6; b++) rhs[b] -= B[6 * a + b] * da;
        }
    }
    solve6_spd(S, rhs, lm_lambda(st->lambdaLg10), dP);
    double dn = 0., pn = 0.;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double p0 = vpose[6 * v + i];
        param[i] = p0 - dP[i];
        dn += dP[i] * dP[i];
        pn += p0 * p0;
    }
    double e2 = 0., R[9];
    cal_rotation_value(param, R);
    const int nres = 8 * cnt;
    for (int r = lane; r < nres; r += 64) {
        const int k = r >> 3, q = (r >> 1) & 3, su = r & 1, o = off + k;
        const int slot = oslot[o];
        const double *cr = crt + 12 * slot;
        const double h = mrt[(size_t)BLD_MR * slot + 39];
        const double X = (q == 0 || q == 3) ? -h : h, Y = q < 2 ? h : -h;
        double P[3];
#pragma unroll
        for (int a = 0; a < 3; a++) P[a] = cr[3 * a] * X + cr[3 * a + 1] * Y + cr[9 + a];
        const double err = cal_project<MODEL>(P, R, param + 3, cam.K, cam.D, su) - (double)markers[omk[o]].corners[2 * q + su];
        e2 += err * err;
    }
    e2 = wave_sum_f64(e2);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) vcand[6 * v + i] = param[i];
        vccost[v] = e2;
        dnpn[2 * v] = dn;
        dnpn[2 * v + 1] = pn;
    }
}

// ------------------------------------------------------------------------------------------------ accept or reject, the stop
__global__ __launch_bounds__(256) void k_build_accept(const BldCfg *__restrict__ cfg, BldState *__restrict__ st, const int *__restrict__ vcnt,
                                                       const int *__restrict__ mfree, double *__restrict__ vpose, const double *__restrict__ vcand,
                                                       const double *__restrict__ vccost, const double *__restrict__ dnpn, double *__restrict__ mpar,
                                                       const double *__restrict__ mcand)
{
    __shared__ double buf[256];
    const int t = threadIdx.x, nv = cfg->n_views;
    if (st->done) return;
    const bool bad = st->bad != 0;
    double cc = 0., dn = 0., pn = 0.;
    for (int v = t; v < nv; v += 256)
        if (vcnt[v] > 0 && !bad) {
            cc += vccost[v];
            dn += dnpn[2 * v];
            pn += dnpn[2 * v + 1];
        }
    cc = bld_sum256(cc, buf, t);
    dn = bld_sum256(dn, buf, t) + st->dnM;
    pn = bld_sum256(pn, buf, t) + st->pnM;
    int l = st->lambdaLg10, done = 0, status = FID_BUILD_OK;
    const int trials = st->trials + 1;
    const bool accept = !bad && cc - cc == 0. && !(cc > st->cost);
    __syncthreads();  // (everything of the state has been read)
    if (accept) {
        for (int i = t; i < 6 * nv; i += 256)
            if (vcnt[i / 6] > 0) vpose[i] = vcand[i];
        for (int i = t; i < 6 * cfg->n_slots; i += 256)
            if (mfree[i / 6] >= 0) mpar[i] = mcand[i];
        l = l - 1 > -16 ? l - 1 : -16;
        if (sqrt(dn) / (sqrt(pn) + DBL_EPSILON) < cfg->eps) done = 1;
    } else {
        l++;
        if (l > 16) {
            l = 16;
            done = 1;
            status = FID_BUILD_STALLED;
        }
    }
    if (!done && trials >= cfg->max_iter) {
        done = 1;
        status = FID_BUILD_MAX_ITER;
    }
    if (t == 0) {
        if (accept) st->cost = cc;
        st->needJ = accept ? 1 : 0;
        st->lambdaLg10 = l;
        st->trials = trials;
        st->status = status;
        st->done = done;
    }
}

// ------------------------------------------------------------------------------------------------ after the stop: the records
__global__ __launch_bounds__(256) void k_build_finish(const BldCfg *__restrict__ cfg, BldState *__restrict__ st, const int *__restrict__ vcnt,
                                                       const double *__restrict__ vcost, const double *__restrict__ vpose, fid_build_out *__restrict__ out,
                                                       fid_build_view *__restrict__ vout)
{
    __shared__ double buf[256];
    const int t = threadIdx.x, nv = cfg->n_views;
    double cs = 0.;
    for (int v = t; v < nv; v += 256)
        if (vcnt[v] > 0) cs += vcost[v];
    cs = bld_sum256(cs, buf, t);
    if (t == 0) {
        st->ctot = cs;
        out->status = st->status;
        out->n_views_used = cfg->n_views_used;
        out->n_markers = cfg->n_slots;
        out->n_fixed = cfg->n_slots - cfg->n_fm;
        out->n_points = cfg->n_points;
        out->n_iter = st->trials;
        out->n_free = cfg->n_free;
        out->reserved0 = 0;
        out->cost = cs;
        out->start_cost = st->trials == 0 ? cs : st->start_cost;
        out->rms = cfg->n_points > 0 ? sqrt(cs / (double)cfg->n_points) : 0.;
    }
    for (int v = t; v < nv; v += 256) {  // (status and n_over are the host's)
        const int cnt = vcnt[v];
        fid_build_view o = vout[v];
        o.n_used = cnt > 0 ? cnt : 0;
        for (int i = 0; i < 3; i++) {
            o.rvec[i] = cnt > 0 ? vpose[6 * v + i] : 0.;
            o.tvec[i] = cnt > 0 ? vpose[6 * v + 3 + i] : 0.;
        }
        o.rms = cnt > 0 ? sqrt(vcost[v] / (double)(4 * cnt)) : 0.;
        vout[v] = o;
    }
}

// a workgroup per slot: the marker's rms; for a free marker its 6 x 6 block of the inverse from the factor: L z = e for its six unit
// columns in blocks of 32 rows, then z^T z, each entry one serial sum in row order.  mout[40 s + ..]: cov (36), rms.
__global__ WALKER_WG_ATTR(256, 1024) void k_build_cov(const BldCfg *__restrict__ cfg, const BldState *__restrict__ st, const double *__restrict__ Sm, const double *__restrict__ Dg,
                                                    const int *__restrict__ mfree, const int *__restrict__ moff, const int *__restrict__ mobs,
                                                    const double *__restrict__ oblk, double *__restrict__ mout)
{
    __shared__ double z[6 * FID_BUILD_MAX_MARKERS][6], D[BLD_NB][BLD_NB + 1];
    const int s = blockIdx.x, t = threadIdx.x, n = cfg->n;
    const int fi = mfree[s];
    if (t == 255) {
        double e2 = 0.;
        const int p0 = moff[s], p1 = moff[s + 1];
        for (int p = p0; p < p1; p++) e2 += oblk[(size_t)mobs[p] * BLD_OB + 63];
        mout[40 * s + 36] = p1 > p0 ? sqrt(e2 / (double)(4 * (p1 - p0))) : 0.;
    }
    const int dof = 2 * cfg->n_points - cfg->n_free;
    const double s2 = cfg->sigma_px > 0. ? cfg->sigma_px * cfg->sigma_px : (dof > 0 ? st->ctot / (double)dof : 0.);
    if (fi < 0 || st->bad || !(s2 > 0.)) {
        if (t < 36) mout[40 * s + t] = 0.;
        return;
    }
    const int c0 = 6 * fi;
    for (int e = t; e < 6 * n; e += 256) z[e / 6][e % 6] = (e / 6 == c0 + e % 6) ? 1. : 0.;
    __syncthreads();
    for (int k0 = (c0 / BLD_NB) * BLD_NB; k0 < n; k0 += BLD_NB) {  // (the rows above the marker's are zero)
        const int nb = n - k0 < BLD_NB ? n - k0 : BLD_NB;
        for (int e = t; e < nb * nb; e += 256) {
            const int r = e / nb, c = e - r * nb;
            if (c <= r) D[r][c] = Dg[(size_t)(k0 / BLD_NB) * BLD_NB * BLD_NB + r * BLD_NB + c];
        }
        __syncthreads();
        if (t < 64) {
            for (int j = 0; j < nb; j++) {
                if (t < 6) z[k0 + j][t] = z[k0 + j][t] / D[j][j];
                SR_LDS_SYNC();
                for (int it = t; it < 6 * nb; it += 64) {
                    const int r = it / 6, c = it - 6 * r;
                    if (r > j) z[k0 + r][c] -= D[r][j] * z[k0 + j][c];
                }
                SR_LDS_SYNC();
            }
        }
        __syncthreads();
        for (int it = t; it < 6 * (n - k0 - nb); it += 256) {
            const int r = k0 + nb + it / 6, c = it % 6;
            double sum = z[r][c];
            for (int p = 0; p < nb; p++) sum -= Sm[(size_t)r * n + k0 + p] * z[k0 + p][c];
            z[r][c] = sum;
        }
        __syncthreads();
    }
    if (t < 36) {
        const int a = t / 6, b = t - 6 * a;
        double sum = 0.;
        for (int r = c0; r < n; r++) sum += z[r][a] * z[r][b];
        sum *= s2;
        mout[40 * s + t] = sum - sum == 0. ? sum : 0.;
    }
}

// ------------------------------------------------------------------------------------------------ the trimmed build's two kernels
// (fid_abi.h: "building the map from views that hold wrong detections"; only fid_build_map_robust_cam launches them)
// the distance between an image corner and the projection of the map point P under the view pose Rt (R 9 | t 3)
template <int MODEL>
__device__ __forceinline__ double bld_corner_dist(const double P[3], const double *R, const double t[3], const double K[9], const double kd[12], const float *corner)
{
    const double dx = cal_project<MODEL>(P, R, t, K, kd, 0) - (double)corner[0];
    const double dy = cal_project<MODEL>(P, R, t, K, kd, 1) - (double)corner[1];
    return sqrt(dx * dx + dy * dy);
}

// the larger of two errors, a NaN staying
__device__ __forceinline__ double bld_worse(double d, double o) { return (o > d || o != o) ? o : d; }

// k_build_place_score: a wave per marker to place (blockIdx.x = p), lanes = its hypotheses.  span[4 p ..] = the marker's observations
// [o0, o1) and hypotheses [h0, h1) (at most 64, the host has ranked them).  hyp: 12 doubles a hypothesis, R | t of T_map_fid; hview: its
// view (the tie rule); oidx[2 j ..]: observation j's record in `markers` and its posed view, whose pose is vrt[12 view ..] = R | t.  A
// lane keeps the four map points of the marker under its hypothesis (in LDS) and walks the observations; the LOWER MEDIAN of the
// errors is exact, by the radix select of k_map_pose_robust on the bit pattern of the (non-negative) double, 7 bits a pass, 128
// sixteen-bit counters a lane in LDS ([bucket][lane], 16 KB; an observation count is at most FID_BUILD_MAX_VIEWS = 4 096): nothing is
// stored per (lane, observation) and nothing is rounded.  Then the arg-min over the lanes (score bits, then the lower view) by a
// butterfly.  res[2 p]: the winning hypothesis' index in the marker's list (-1: none), res[2 p + 1]: its score.  (Eight pointers, not
// one per list: with the camera's 21 doubles the arguments alone fill the scalar registers.)
template <int MODEL>
__global__ WALKER_WG_ATTR(64, 1024) void k_build_place_score(PoseCam cam, const fid_marker *__restrict__ markers, const int *__restrict__ span,
                                                           const int *__restrict__ oidx, const double *__restrict__ vrt, const double *__restrict__ hyp,
                                                           const int *__restrict__ hview, const double *__restrict__ half, double *__restrict__ res)
{
    __shared__ unsigned short counters[128 * 64];
    __shared__ double points[12 * 64];  // a lane's four map points ([coordinate][lane]: 24 registers a lane otherwise)
    const int p = blockIdx.x, lane = threadIdx.x;
    const int o0 = span[4 * p], m = span[4 * p + 1] - o0, h0 = span[4 * p + 2];
    int nh = span[4 * p + 3] - h0;
    nh = nh > 64 ? 64 : nh;
    unsigned long long score_bits = ~0ull;
    int view = 0x7fffffff;
    if (lane < nh && m > 0) {
        const double *T = hyp + (size_t)12 * (h0 + lane);
        const double h = half[p];
        double *Pm = points + lane;  // coordinate a of corner q: Pm[64 * (3 q + a)]
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double X = (q == 0 || q == 3) ? -h : h, Y = q < 2 ? h : -h;
#pragma unroll
            for (int a = 0; a < 3; a++) Pm[64 * (3 * q + a)] = T[3 * a] * X + T[3 * a + 1] * Y + T[9 + a];
        }
        view = hview[h0 + lane];
        unsigned short *cnt = counters + lane;  // counter of bucket b: cnt[64 * b]
        unsigned long long prefix = 0ull;
        int rank = (m - 1) / 2, members = m;
        for (int shift = 56; shift >= 0; shift -= 7) {
            for (int b = 0; b < 128; b++) cnt[64 * b] = 0;
            unsigned long long last = 0ull;
            for (int j = 0; j < m; j++) {
                const double *Rt = vrt + (size_t)12 * oidx[2 * (o0 + j) + 1];
                const float *cn = markers[oidx[2 * (o0 + j)]].corners;
                double e = 0.;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const double P[3] = {Pm[64 * (3 * q)], Pm[64 * (3 * q + 1)], Pm[64 * (3 * q + 2)]};
                    e = bld_worse(e, bld_corner_dist<MODEL>(P, Rt, Rt + 9, cam.K, cam.D, cn + 2 * q));
                }
                const unsigned long long bits = (unsigned long long)__double_as_longlong(e) & 0x7fffffffffffffffull;
                if ((bits >> (shift + 7)) == prefix) {
                    last = bits;
                    cnt[64 * (int)((bits >> shift) & 127ull)]++;
                }
            }
            if (members == 1) {  // the prefix has one member: this pass has met it
                prefix = last;
                break;
            }
            int b = 0, below = 0;
            for (; b < 127; b++) {
                const int cb = cnt[64 * b];
                if (below + cb > rank) break;
                below += cb;
            }
            rank -= below;
            members = cnt[64 * b];
            prefix = (prefix << 7) | (unsigned long long)b;
        }
        score_bits = prefix;
    }
    int win_lane = lane;
    for (int mask = 1; mask < 64; mask <<= 1) {
        const unsigned lo = __shfl_xor((unsigned)score_bits, mask, WAVE), hi = __shfl_xor((unsigned)(score_bits >> 32), mask, WAVE);
        const unsigned long long ob = ((unsigned long long)hi << 32) | lo;
        const int ov = __shfl_xor(view, mask, WAVE), ol = __shfl_xor(win_lane, mask, WAVE);
        if (ob < score_bits || (ob == score_bits && (ov < view || (ov == view && ol < win_lane)))) {
            score_bits = ob;
            view = ov;
            win_lane = ol;
        }
    }
    if (lane == 0) {
        res[2 * p] = view == 0x7fffffff ? -1. : (double)win_lane;
        res[2 * p + 1] = __longlong_as_double((long long)score_bits);
    }
}

// k_build_obs_err: a wave per view, a lane per corner of 16 observations at a time; the view's R once into LDS.  evoff / evcnt: the
// view's observations in the dense list; eomk: the observation's record in `markers`; eom: its marker, whose pose is emrt[16 marker ..]
// = R (9) | t (3) | h; evpose: (rvec, tvec) a view.  err[o]: the largest of the four corner distances.
template <int MODEL>
__global__ WALKER_WG_ATTR(64, 1024) void k_build_obs_err(PoseCam cam, const fid_marker *__restrict__ markers, const int *__restrict__ evoff,
                                                       const int *__restrict__ evcnt, const int *__restrict__ eomk, const int *__restrict__ eom,
                                                       const double *__restrict__ emrt, const double *__restrict__ evpose, double *__restrict__ err)
{
    __shared__ double rot[36], rtmp[80];
    const int v = blockIdx.x, lane = threadIdx.x;
    const int cnt = evcnt[v], off = evoff[v];
    if (cnt <= 0) return;
    cal_rotation_lds(evpose + 6 * v, rot, rtmp, lane);
    SR_LDS_SYNC();
    double tv[3];
#pragma unroll
    for (int i = 0; i < 3; i++) tv[i] = evpose[6 * v + 3 + i];
    for (int k0 = 0; k0 < cnt; k0 += 16) {
        const int k = k0 + (lane >> 2), q = lane & 3;
        double d = 0.;
        if (k < cnt) {
            const int o = off + k;
            const double *mr = emrt + (size_t)16 * eom[o];
            const double h = mr[12];
            const double X = (q == 0 || q == 3) ? -h : h, Y = q < 2 ? h : -h;
            double P[3];
#pragma unroll
            for (int a = 0; a < 3; a++) P[a] = mr[3 * a] * X + mr[3 * a + 1] * Y + mr[9 + a];
            d = bld_corner_dist<MODEL>(P, rot, tv, cam.K, cam.D, markers[eomk[o]].corners + 2 * q);
        }
        d = bld_worse(d, shfl_xor_f64(d, 1));
        d = bld_worse(d, shfl_xor_f64(d, 2));
        if (q == 0 && k < cnt) err[off + k] = d;
    }
}

// ------------------------------------------------------------------------------------------------ host
struct BuildBufs : DevBlock {};

static void build_free(fid_ctx *c)
{
    delete c->build;
    c->build = nullptr;
}

void fid_default_build_opts(fid_build_opts *o)
{
    if (!o) return;
    o->fiducial_len = 0.;
    o->len_ids = nullptr;
    o->len_values = nullptr;
    o->n_len = 0;
    o->min_views = 2;
    o->max_iter = 100;
    o->reserved0 = 0;
    o->eps = 1e-12;
    o->sigma_px = 0.;
}

namespace {

void bld_rod_v2m(const double r[3], double R[9])
{
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1. : 0.;
    if (th < DBL_EPSILON) return;
    const double k[3] = {r[0] / th, r[1] / th, r[2] / th}, sn = sin(th), c1 = 1. - cos(th);
    const double kx[9] = {0., -k[2], k[1], k[2], 0., -k[0], -k[1], k[0], 0.};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double kk = kx[3 * i] * kx[j] + kx[3 * i + 1] * kx[3 + j] + kx[3 * i + 2] * kx[6 + j];
            R[3 * i + j] = ((i == j ? 1. : 0.) + sn * kx[3 * i + j]) + c1 * kk;
        }
}

// rotation matrix -> vector (cvRodrigues2's matrix branch without the SVD: the input is a product of rotations)
void bld_rod_m2v(const double R[9], double r[3])
{
    const double ax[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double s = sqrt((ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1.) * 0.5;
    c = c > 1. ? 1. : (c < -1. ? -1. : c);
    const double th = acos(c);
    if (s < 1e-5) {
        if (c > 0.) {
            r[0] = r[1] = r[2] = 0.;
            return;
        }
        double t0 = sqrt(fmax((R[0] + 1.) * 0.5, 0.)), t1 = sqrt(fmax((R[4] + 1.) * 0.5, 0.)) * (R[1] < 0. ? -1. : 1.),
               t2 = sqrt(fmax((R[8] + 1.) * 0.5, 0.)) * (R[2] < 0. ? -1. : 1.);
        if (fabs(t0) < fabs(t1) && fabs(t0) < fabs(t2) && (R[5] > 0.) != (t1 * t2 > 0.)) t2 = -t2;
        const double nrm = th / sqrt(t0 * t0 + t1 * t1 + t2 * t2);
        r[0] = t0 * nrm;
        r[1] = t1 * nrm;
        r[2] = t2 * nrm;
        return;
    }
    const double vth = 0.5 / s * th;
    for (int i = 0; i < 3; i++) r[i] = ax[i] * vth;
}

bool bld_finite(double x) { return x - x == 0.; }

}  // namespace

// One call of either entry point, in the steps both share: check (the arguments), select (the kept observations, the id table), plan
// (FEW_VIEWS and reachability over the active observations), alloc (the context's buffer), stage (the markers up, k_pose over them),
// the start (start_plain, or start_robust with its two helpers), solve (Levenberg-Marquardt over the active observations from the
// poses held here, and the records into a BldResult).  fid_build_map_cam is check, select, plan, alloc, stage, start_plain, solve;
// fid_build_map_robust_cam runs solve in rounds with obs_err and plan between them.
namespace {

struct BldResult {
    fid_build_out out;
    std::vector<fid_build_view> views;
    std::vector<fid_build_marker> markers;
    std::vector<std::vector<char>> active;   // the set the solve ran over, as BldRun::active
    std::vector<std::vector<double>> err;    // err per kept observation under these parameters, -1 where it has none
    int n_obs = 0;
};

struct BldRun {
    fid_ctx *c;
    const char *who;
    const fid_marker *markers;
    const int32_t *n_per_view;
    int V, cap_per_view;
    const fid_map_entry *fixed;
    int n_fixed;
    const fid_build_opts *opts;
    fid_camera cam;
    PoseCam pcam;
    // select
    std::vector<std::vector<int>> kept, kid;  // a view's kept markers: list positions, id indices
    std::vector<std::vector<char>> active;
    std::vector<int> n_over, ids, fix_of, nview;
    std::vector<double> len;
    int NI = 0;
    // plan
    std::vector<int> mstatus, vstatus;
    std::vector<char> cand, placed, reached;
    int n_in = 0, n_reached = 0;
    // the poses: the start's, then every solve's
    std::vector<char> has_vpose, has_mpose, has_mrv;
    std::vector<double> vpose, mR, mt, mrv;  // 6 a view; 9, 3 and (after a solve) the six parameters a marker
    std::vector<fid_pose_out> p1;
    // the buffer
    bool robust = false;
    int pv = 1, NS = 0;
    size_t VP = 0, n_obs_max = 1, off_solve0 = 0, off_solve1 = 0;
    char *M = nullptr;
    BldCfg *d_cfg;
    BldState *d_state;
    fid_build_out *d_out;
    fid_marker *d_mk;
    int *d_n, *d_tid, *d_voff, *d_vcnt, *d_omk, *d_oslot, *d_oview, *d_mobs, *d_moff, *d_mfree, *d_fslot;
    double *d_lens, *d_tobj, *d_mpar, *d_mcand, *d_mrt, *d_crt, *d_mout, *d_vpose, *d_vcand, *d_vblk, *d_vcost, *d_vccost, *d_dnpn, *d_oblk, *d_ow, *d_S, *d_Dg, *d_g,
        *d_dx;
    fid_pose_out *d_p1;
    fid_map_pose_out *d_mp;
    fid_build_view *d_vout;
    // the trimmed build's part of it
    fid_map_robust_out *d_rob;
    int *d_pspan, *d_poidx, *d_phview, *d_evoff, *d_evcnt, *d_eomk, *d_eom;
    double *d_vrt, *d_hyp, *d_phalf, *d_pres, *d_emrt, *d_evpose, *d_err;
    std::vector<int> evoff, evcnt;  // the dense list of the observations that have an err: view v's [evoff, evoff + evcnt), in kept order
    int n_err = 0;

    bool refuse(const std::string &why)
    {
        c->last_error = std::string(who) + ": " + why;
        return true;
    }

    fid_status check(const fid_camera *camera, fid_build_out *out, fid_build_marker *markers_out, int32_t cap_markers, int32_t *n_markers_out)
    {
        if (n_markers_out) *n_markers_out = 0;
        if (!camera || !markers || !n_per_view || !fixed || !opts || !out || !n_markers_out || (cap_markers > 0 && !markers_out))
            return refuse("a NULL pointer"), FID_E_INVALID_ARG;
        if (V < 1 || V > FID_BUILD_MAX_VIEWS)
            return refuse(std::to_string(V) + " views: 1 .. " + std::to_string(FID_BUILD_MAX_VIEWS) + " (FID_BUILD_MAX_VIEWS)"), FID_E_INVALID_ARG;
        if (cap_per_view < 1 || cap_markers < 0) return refuse("cap_per_view must be positive, cap_markers not negative"), FID_E_INVALID_ARG;
        if (!fid_camera_usable(camera)) return refuse("the camera's model or n_dist is outside the ABI's"), FID_E_INVALID_ARG;
        if (n_fixed < 1) return refuse("no fixed entry: at least one fiducial must define the map frame"), FID_E_INVALID_ARG;
        if (!(opts->eps >= 0.) || !bld_finite(opts->eps) || !(opts->sigma_px >= 0.) || !bld_finite(opts->sigma_px) || opts->max_iter < 0 || opts->min_views < 1 ||
            opts->n_len < 0 || (opts->n_len > 0 && (!opts->len_ids || !opts->len_values)))
            return refuse("eps and sigma_px must be finite and >= 0, max_iter >= 0, min_views >= 1, n_len >= 0 with its lists"), FID_E_INVALID_ARG;
        if (!(opts->fiducial_len > 0.) || !bld_finite(opts->fiducial_len)) return refuse("fiducial_len must be positive"), FID_E_INVALID_ARG;
        for (int k = 0; k < opts->n_len; k++)
            if (!(opts->len_values[k] > 0.) || !bld_finite(opts->len_values[k]))
                return refuse("the length given for id " + std::to_string(opts->len_ids[k]) + " must be positive"), FID_E_INVALID_ARG;
        cam = fid_camera_normalised(*camera);
        for (int i = 0; i < 9; i++)
            if (!bld_finite(cam.K[i])) return refuse("the camera holds a value that is not finite"), FID_E_INVALID_ARG;
        for (int i = 0; i < 12; i++)
            if (!bld_finite(cam.D[i])) return refuse("the camera holds a value that is not finite"), FID_E_INVALID_ARG;
        std::vector<int> fix_order((size_t)n_fixed);
        for (int i = 0; i < n_fixed; i++) {
            fix_order[(size_t)i] = i;
            const fid_map_entry &e = fixed[i];
            bool fin = bld_finite(e.len);
            for (int k = 0; k < 9; k++) fin = fin && bld_finite(e.R[k]);
            for (int k = 0; k < 3; k++) fin = fin && bld_finite(e.t[k]);
            if (!(e.len > 0.) || !fin)
                return refuse("fixed entry " + std::to_string(i) + " (id " + std::to_string(e.id) + "): len must be positive and the transform finite"),
                       FID_E_INVALID_ARG;
        }
        std::sort(fix_order.begin(), fix_order.end(), [&](int a, int b) { return fixed[a].id < fixed[b].id; });
        for (int i = 1; i < n_fixed; i++)
            if (fixed[fix_order[(size_t)i]].id == fixed[fix_order[(size_t)i - 1]].id)
                return refuse("fixed: id " + std::to_string(fixed[fix_order[(size_t)i]].id) + " is listed twice"), FID_E_INVALID_ARG;
        if (refuse_in_flight(c)) return FID_E_INVALID_ARG;
        return FID_OK;
    }

    // ---- the views' kept markers (list order, an id seen twice left out, the first FID_BUILD_MAX_PER_VIEW), the id table
    fid_status select(int32_t cap_markers, int32_t *n_markers_out)
    {
        kept.assign((size_t)V, {});
        n_over.assign((size_t)V, 0);
        for (int v = 0; v < V; v++) {
            const int n = n_per_view[v] < 0 ? 0 : (n_per_view[v] > cap_per_view ? cap_per_view : n_per_view[v]);
            const fid_marker *m = markers + (size_t)v * cap_per_view;
            std::vector<int> vid((size_t)n);
            for (int i = 0; i < n; i++) {
                for (int q = 0; q < 8; q++)
                    if (m[i].corners[q] - m[i].corners[q] != 0.f)
                        return refuse("view " + std::to_string(v) + ", marker " + std::to_string(i) + ": a corner is not finite"), FID_E_INVALID_ARG;
                vid[(size_t)i] = m[i].id;
            }
            std::vector<int> sorted = vid;
            std::sort(sorted.begin(), sorted.end());
            for (int i = 0; i < n; i++) {
                const auto range = std::equal_range(sorted.begin(), sorted.end(), vid[(size_t)i]);
                if (range.second - range.first != 1) continue;
                if ((int)kept[(size_t)v].size() < FID_BUILD_MAX_PER_VIEW) {
                    kept[(size_t)v].push_back(i);
                    ids.push_back(vid[(size_t)i]);
                } else {
                    n_over[(size_t)v]++;
                }
            }
        }
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        NI = (int)ids.size();
        *n_markers_out = NI;
        if (NI > cap_markers)
            return refuse(std::to_string(NI) + " ids are seen, markers_out has room for " + std::to_string(cap_markers)), FID_E_CAPACITY;
        fix_of.assign((size_t)NI, -1);
        nview.assign((size_t)NI, 0);
        len.assign((size_t)NI, opts->fiducial_len);
        for (int i = 0; i < n_fixed; i++) {
            const auto it = std::lower_bound(ids.begin(), ids.end(), fixed[i].id);
            if (it != ids.end() && *it == fixed[i].id) fix_of[(size_t)(it - ids.begin())] = i;
        }
        for (int m = 0; m < NI; m++) {
            for (int k = opts->n_len - 1; k >= 0; k--)
                if (opts->len_ids[k] == ids[(size_t)m]) len[(size_t)m] = opts->len_values[k];
            if (fix_of[(size_t)m] >= 0) len[(size_t)m] = fixed[fix_of[(size_t)m]].len;
        }
        kid.assign((size_t)V, {});
        active.assign((size_t)V, {});
        for (int v = 0; v < V; v++)
            for (int pos : kept[(size_t)v]) {
                const int m = (int)(std::lower_bound(ids.begin(), ids.end(), markers[(size_t)v * cap_per_view + pos].id) - ids.begin());
                kid[(size_t)v].push_back(m);
                active[(size_t)v].push_back(1);
                nview[(size_t)m]++;
            }
        return FID_OK;
    }

    // ---- FEW_VIEWS, then reachability as a fixed point, over the active observations.  false: no reached view
    bool plan()
    {
        std::vector<int> nact((size_t)NI, 0);
        for (int v = 0; v < V; v++)
            for (size_t k = 0; k < kid[(size_t)v].size(); k++)
                if (active[(size_t)v][k]) nact[(size_t)kid[(size_t)v][k]]++;
        mstatus.assign((size_t)NI, FID_BUILD_MARKER_UNREACHED);
        cand.assign((size_t)NI, 0);
        placed.assign((size_t)NI, 0);
        reached.assign((size_t)V, 0);
        for (int m = 0; m < NI; m++) {
            if (fix_of[(size_t)m] >= 0) {
                cand[(size_t)m] = placed[(size_t)m] = 1;
            } else if (nact[(size_t)m] < opts->min_views) {
                mstatus[(size_t)m] = FID_BUILD_MARKER_FEW_VIEWS;
            } else {
                cand[(size_t)m] = 1;
            }
        }
        auto holds = [&](int v, const std::vector<char> &set) {
            for (size_t k = 0; k < kid[(size_t)v].size(); k++)
                if (active[(size_t)v][k] && set[(size_t)kid[(size_t)v][k]]) return true;
            return false;
        };
        for (bool changed = true; changed;) {
            changed = false;
            for (int v = 0; v < V; v++) {
                if (reached[(size_t)v] || !holds(v, placed)) continue;
                reached[(size_t)v] = 1;
                changed = true;
                for (size_t k = 0; k < kid[(size_t)v].size(); k++)
                    if (active[(size_t)v][k] && cand[(size_t)kid[(size_t)v][k]]) placed[(size_t)kid[(size_t)v][k]] = 1;
            }
        }
        vstatus.assign((size_t)V, FID_BUILD_VIEW_UNREACHED);
        n_in = n_reached = 0;
        for (int m = 0; m < NI; m++) n_in += placed[(size_t)m] ? 1 : 0;
        for (int v = 0; v < V; v++) {
            if (!holds(v, cand)) vstatus[(size_t)v] = FID_BUILD_VIEW_FEW;
            if (reached[(size_t)v]) n_reached++;
        }
        return n_reached > 0;
    }

    // ---- the device buffer: the plain call's, and behind it what only the trimmed build uses
    fid_status alloc()
    {
        NS = n_in;
        pv = 1;
        for (int v = 0; v < V; v++) pv = std::max(pv, (int)kept[(size_t)v].size());
        n_obs_max = 0;
        for (int v = 0; v < V; v++) n_obs_max += kept[(size_t)v].size();
        n_obs_max = std::max<size_t>(n_obs_max, 1);
        const size_t nmax = 6 * (size_t)NS, S1 = (size_t)NS + 1, O = n_obs_max;
        VP = (size_t)V * pv;
        MemLayout l;
        l.add(&d_cfg, 1), l.add(&d_state, 1), l.add(&d_out, 1), l.add(&d_mk, VP), l.add(&d_n, V), l.add(&d_lens, VP), l.add(&d_p1, VP), l.add(&d_mp, V);
        off_solve0 = l.mark();
        l.add(&d_tid, S1), l.add(&d_tobj, 12 * S1), l.add(&d_voff, V), l.add(&d_vcnt, V), l.add(&d_omk, O), l.add(&d_oslot, O), l.add(&d_oview, O);
        l.add(&d_mobs, O), l.add(&d_moff, S1), l.add(&d_mfree, S1), l.add(&d_fslot, S1), l.add(&d_mpar, 6 * S1), l.add(&d_mcand, 6 * S1);
        l.add(&d_mrt, BLD_MR * S1), l.add(&d_crt, 12 * S1), l.add(&d_mout, 40 * S1), l.add(&d_vout, V), l.add(&d_vpose, 6 * (size_t)V);
        l.add(&d_vcand, 6 * (size_t)V), l.add(&d_vblk, BLD_VB * (size_t)V), l.add(&d_vcost, V), l.add(&d_vccost, V), l.add(&d_dnpn, 2 * (size_t)V);
        l.add(&d_oblk, BLD_OB * O), l.add(&d_ow, BLD_OW * O), l.add(&d_S, std::max<size_t>(nmax * nmax, 1)), l.add(&d_g, nmax + 1), l.add(&d_dx, nmax + 1);
        l.add(&d_Dg, BLD_NB * BLD_NB * (nmax / BLD_NB + 1));
        off_solve1 = l.mark();
        if (robust) {
            l.add(&d_rob, V), l.add(&d_pspan, 4 * S1), l.add(&d_poidx, 2 * O), l.add(&d_phview, O), l.add(&d_evoff, V), l.add(&d_evcnt, V), l.add(&d_eomk, O);
            l.add(&d_eom, O), l.add(&d_vrt, 12 * (size_t)V), l.add(&d_hyp, 12 * O), l.add(&d_phalf, S1), l.add(&d_pres, 2 * S1);
            l.add(&d_emrt, 16 * ((size_t)NI + 1)), l.add(&d_evpose, 6 * (size_t)V), l.add(&d_err, O);
        }
        const size_t off = l.bytes();
        HIPCHK(c, hipSetDevice(c->device));
        if (!c->build) c->build = new (std::nothrow) BuildBufs();
        if (!c->build) return FID_E_OUT_OF_MEMORY;
        HIPCHK(c, c->build->reserve(off));
        M = c->build->p;
        l.bind(M);
        HIPCHK(c, hipMemsetAsync(M, 0, off, c->stream));
        return FID_OK;
    }

    // ---- the markers up, k_pose once over all kept markers, the fixed markers' places
    fid_status stage()
    {
        hipStream_t st = c->stream;
        std::vector<fid_marker> hmk(VP);
        std::vector<double> hlens(VP, opts->fiducial_len);
        std::vector<int> hn((size_t)V);
        memset(hmk.data(), 0, sizeof(fid_marker) * VP);
        for (int v = 0; v < V; v++) {
            hn[(size_t)v] = (int)kept[(size_t)v].size();
            for (size_t k = 0; k < kept[(size_t)v].size(); k++) {
                hmk[(size_t)v * pv + k] = markers[(size_t)v * cap_per_view + kept[(size_t)v][k]];
                hlens[(size_t)v * pv + k] = len[(size_t)kid[(size_t)v][k]];
            }
        }
        HIPCHK(c, hipMemcpyAsync(d_mk, hmk.data(), sizeof(fid_marker) * VP, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_lens, hlens.data(), sizeof(double) * VP, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_n, hn.data(), sizeof(int) * V, hipMemcpyHostToDevice, st));
        pcam = pose_cam_from(cam, opts->fiducial_len);
        {
            int blocks = (int)((VP + 7) / 8);
            blocks = blocks < 1 ? 1 : (blocks > 256 * 16 ? 256 * 16 : blocks);
            POSE_CAM_DISPATCH(pcam.model, hipLaunchKernelGGL(k_pose<CAM_MODEL>, dim3(blocks), dim3(64), 0, st, (const fid_marker *)d_mk, (const int *)d_n, 1,
                                                             (const double *)d_lens, V, pv, pcam, d_p1));
        }
        HIPCHK(c, hipGetLastError());
        p1.resize(VP);
        HIPCHK(c, hipMemcpyAsync(p1.data(), d_p1, sizeof(fid_pose_out) * VP, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        has_vpose.assign((size_t)V, 0);
        has_mpose.assign((size_t)NI, 0);
        has_mrv.assign((size_t)NI, 0);
        vpose.assign((size_t)V * 6, 0.);
        mR.assign((size_t)NI * 9, 0.);
        mt.assign((size_t)NI * 3, 0.);
        mrv.assign((size_t)NI * 6, 0.);
        for (int m = 0; m < NI; m++) {
            const int f = fix_of[(size_t)m];
            if (f < 0 || !placed[(size_t)m]) continue;
            has_mpose[(size_t)m] = 1;
            for (int k = 0; k < 9; k++) mR[(size_t)m * 9 + k] = fixed[f].R[k];
            for (int k = 0; k < 3; k++) mt[(size_t)m * 3 + k] = fixed[f].t[k];
        }
        return FID_OK;
    }

    bool holds_placed(int v) const
    {
        for (int m : kid[(size_t)v])
            if (placed[(size_t)m] && has_mpose[(size_t)m]) return true;
        return false;
    }
    bool wants_pose(int v) const { return !has_vpose[(size_t)v] && vstatus[(size_t)v] != FID_BUILD_VIEW_NO_START && reached[(size_t)v]; }

    // (a) of a start round: the placed markers in the solve as a map (ids ascending), the views' solve by `launch`, which leaves one
    // record a view in mp and says per view whether it holds a pose
    template <typename Launch, typename Ok>
    fid_status start_views(std::vector<fid_map_pose_out> &mp, Launch launch, Ok ok_of, bool *changed)
    {
        hipStream_t st = c->stream;
        bool want = false;
        for (int v = 0; v < V && !want; v++) want = wants_pose(v) && holds_placed(v);
        if (!want) return FID_OK;
        std::vector<int> tid;
        std::vector<double> tobj;
        for (int m = 0; m < NI; m++) {
            if (!placed[(size_t)m] || !has_mpose[(size_t)m]) continue;
            tid.push_back(ids[(size_t)m]);
            const double h = (double)(float)(len[(size_t)m] / 2);
            const double cx[4] = {-h, h, h, -h}, cy[4] = {h, h, -h, -h};
            for (int q = 0; q < 4; q++)
                for (int a = 0; a < 3; a++) tobj.push_back(mR[(size_t)m * 9 + 3 * a] * cx[q] + mR[(size_t)m * 9 + 3 * a + 1] * cy[q] + mt[(size_t)m * 3 + a]);
        }
        HIPCHK(c, hipMemcpyAsync(d_tid, tid.data(), sizeof(int) * tid.size(), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_tobj, tobj.data(), sizeof(double) * tobj.size(), hipMemcpyHostToDevice, st));
        const fid_status rc = launch((int)tid.size());
        if (rc != FID_OK) return rc;
        for (int v = 0; v < V; v++) {
            if (!wants_pose(v) || !holds_placed(v)) continue;
            const fid_map_pose_out &o = mp[(size_t)v];
            bool ok = ok_of(v) && o.n_markers > 0 && o.image_error >= 0.;
            for (int i = 0; i < 3; i++) ok = ok && bld_finite(o.rvec[i]) && bld_finite(o.tvec[i]);
            *changed = true;
            if (!ok) {
                vstatus[(size_t)v] = FID_BUILD_VIEW_NO_START;
                continue;
            }
            has_vpose[(size_t)v] = 1;
            for (int i = 0; i < 3; i++) {
                vpose[(size_t)v * 6 + i] = o.rvec[i];
                vpose[(size_t)v * 6 + 3 + i] = o.tvec[i];
            }
        }
        return FID_OK;
    }

    bool pose_usable(const fid_pose_out &p) const
    {
        bool ok = p.image_error >= 0. && bld_finite(p.fiducial_area);
        for (int i = 0; i < 3; i++) ok = ok && bld_finite(p.rvec[i]) && bld_finite(p.tvec[i]);
        return ok;
    }

    // T_map_fid = T_cam_map(v)^-1 T_cam_fid(p): R (9) and t (3)
    void compose(int v, const fid_pose_out &p, double *R, double *t) const
    {
        double Rcm[9], Rcf[9];
        bld_rod_v2m(&vpose[(size_t)v * 6], Rcm);
        bld_rod_v2m(p.rvec, Rcf);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) R[3 * i + j] = Rcm[i] * Rcf[j] + Rcm[3 + i] * Rcf[3 + j] + Rcm[6 + i] * Rcf[6 + j];
            t[i] = Rcm[i] * (p.tvec[0] - vpose[(size_t)v * 6 + 3]) + Rcm[3 + i] * (p.tvec[1] - vpose[(size_t)v * 6 + 4]) + Rcm[6 + i] * (p.tvec[2] - vpose[(size_t)v * 6 + 5]);
        }
    }

    // ---- the start: k_map_pose per round over the placed markers, a marker from the posed view where its image area is largest
    fid_status start_plain()
    {
        hipStream_t st = c->stream;
        std::vector<fid_map_pose_out> mp((size_t)V);
        for (bool changed = true; changed;) {
            changed = false;
            const fid_status rc = start_views(
                mp,
                [&](int n_map) -> fid_status {
                    POSE_CAM_DISPATCH(pcam.model, hipLaunchKernelGGL(k_map_pose<CAM_MODEL>, dim3(V), dim3(64), 0, st, (const fid_marker *)d_mk, (const int *)d_n, 1, pv,
                                                                     (const int *)d_tid, (const double *)d_tobj, n_map, pcam, d_mp));
                    HIPCHK(c, hipGetLastError());
                    HIPCHK(c, hipMemcpyAsync(mp.data(), d_mp, sizeof(fid_map_pose_out) * V, hipMemcpyDeviceToHost, st));
                    HIPCHK(c, hipStreamSynchronize(st));
                    return FID_OK;
                },
                [](int) { return true; }, &changed);
            if (rc != FID_OK) return rc;
            // (b) the markers that a posed view keeps: from the view where their image area is largest
            for (int m = 0; m < NI; m++) {
                if (!placed[(size_t)m] || has_mpose[(size_t)m]) continue;
                int bv = -1, bk = -1;
                double best = -1.;
                for (int v = 0; v < V; v++) {
                    if (!has_vpose[(size_t)v]) continue;
                    for (size_t k = 0; k < kid[(size_t)v].size(); k++) {
                        if (kid[(size_t)v][k] != m) continue;
                        const fid_pose_out &p = p1[(size_t)v * pv + k];
                        if (pose_usable(p) && p.fiducial_area > best) {
                            best = p.fiducial_area;
                            bv = v;
                            bk = (int)k;
                        }
                    }
                }
                if (bv < 0) continue;
                compose(bv, p1[(size_t)bv * pv + bk], &mR[(size_t)m * 9], &mt[(size_t)m * 3]);
                has_mpose[(size_t)m] = 1;
                changed = true;
            }
        }
        return FID_OK;
    }

    // ---- the robust start (fid_abi.h): k_map_pose_robust per round, a marker from the hypothesis of smallest median err
    fid_status start_robust(const fid_build_robust_opts &ro)
    {
        hipStream_t st = c->stream;
        std::vector<fid_map_pose_out> mp((size_t)V);
        std::vector<fid_map_robust_out> rob((size_t)V);
        for (bool changed = true; changed;) {
            changed = false;
            const fid_status rc = start_views(
                mp,
                [&](int n_map) -> fid_status {
                    POSE_CAM_DISPATCH(pcam.model, hipLaunchKernelGGL(k_map_pose_robust<CAM_MODEL>, dim3(V), dim3(64), 0, st, (const fid_marker *)d_mk, (const int *)d_n, 1,
                                                                     pv, (const int *)d_tid, (const double *)d_tobj, n_map, pcam, ro.inlier_px, 1, d_mp, d_rob));
                    HIPCHK(c, hipGetLastError());
                    HIPCHK(c, hipMemcpyAsync(mp.data(), d_mp, sizeof(fid_map_pose_out) * V, hipMemcpyDeviceToHost, st));
                    HIPCHK(c, hipMemcpyAsync(rob.data(), d_rob, sizeof(fid_map_robust_out) * V, hipMemcpyDeviceToHost, st));
                    HIPCHK(c, hipStreamSynchronize(st));
                    return FID_OK;
                },
                [&](int v) { return rob[(size_t)v].status == FID_MAP_ROBUST_OK; }, &changed);
            if (rc != FID_OK) return rc;
            // (b) the hypotheses of every marker that enough posed views keep, scored in one launch
            struct Hyp {
                double area;
                int v, k;
            };
            std::vector<int> pm, pspan, poidx, phview;
            std::vector<double> hyp, phalf;
            for (int m = 0; m < NI; m++) {
                if (!placed[(size_t)m] || has_mpose[(size_t)m]) continue;
                std::vector<Hyp> hs;
                const size_t o_before = poidx.size();
                for (int v = 0; v < V; v++) {
                    if (!has_vpose[(size_t)v]) continue;
                    for (size_t k = 0; k < kid[(size_t)v].size(); k++) {
                        if (kid[(size_t)v][k] != m) continue;
                        poidx.push_back(v * pv + (int)k);
                        poidx.push_back(v);
                        const fid_pose_out &p = p1[(size_t)v * pv + k];
                        if (pose_usable(p)) hs.push_back({p.fiducial_area, v, (int)k});
                    }
                }
                if ((int)((poidx.size() - o_before) / 2) < ro.min_views_place || hs.empty()) {
                    poidx.resize(o_before);
                    continue;
                }
                std::stable_sort(hs.begin(), hs.end(), [](const Hyp &a, const Hyp &b) { return a.area > b.area; });  // (equal areas stay in view order)
                if (hs.size() > FID_BUILD_ROBUST_HYPOTHESES) hs.resize(FID_BUILD_ROBUST_HYPOTHESES);
                const int h_before = (int)phview.size();
                for (const Hyp &h : hs) {
                    double T[12];
                    compose(h.v, p1[(size_t)h.v * pv + h.k], T, T + 9);
                    hyp.insert(hyp.end(), T, T + 12);
                    phview.push_back(h.v);
                }
                pm.push_back(m);
                const int span4[4] = {(int)(o_before / 2), (int)(poidx.size() / 2), h_before, (int)phview.size()};
                pspan.insert(pspan.end(), span4, span4 + 4);
                phalf.push_back((double)(float)(len[(size_t)m] / 2));
            }
            const int NP = (int)pm.size();
            if (NP == 0) continue;
            std::vector<double> vrt((size_t)V * 12, 0.);
            for (int v = 0; v < V; v++) {
                if (!has_vpose[(size_t)v]) continue;
                bld_rod_v2m(&vpose[(size_t)v * 6], &vrt[(size_t)v * 12]);
                for (int i = 0; i < 3; i++) vrt[(size_t)v * 12 + 9 + i] = vpose[(size_t)v * 6 + 3 + i];
            }
            HIPCHK(c, hipMemcpyAsync(d_pspan, pspan.data(), sizeof(int) * pspan.size(), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_poidx, poidx.data(), sizeof(int) * poidx.size(), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_phview, phview.data(), sizeof(int) * phview.size(), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_hyp, hyp.data(), sizeof(double) * hyp.size(), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_phalf, phalf.data(), sizeof(double) * phalf.size(), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_vrt, vrt.data(), sizeof(double) * vrt.size(), hipMemcpyHostToDevice, st));
            POSE_CAM_DISPATCH(pcam.model, hipLaunchKernelGGL(k_build_place_score<CAM_MODEL>, dim3(NP), dim3(64), 0, st, pcam, (const fid_marker *)d_mk, (const int *)d_pspan,
                                                             (const int *)d_poidx, (const double *)d_vrt, (const double *)d_hyp, (const int *)d_phview,
                                                             (const double *)d_phalf, d_pres));
            HIPCHK(c, hipGetLastError());
            std::vector<double> pres((size_t)NP * 2);
            HIPCHK(c, hipMemcpyAsync(pres.data(), d_pres, sizeof(double) * 2 * NP, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            for (int p = 0; p < NP; p++) {
                const int b = (int)pres[(size_t)2 * p], m = pm[(size_t)p];
                if (b < 0 || b >= pspan[(size_t)4 * p + 3] - pspan[(size_t)4 * p + 2] || !bld_finite(pres[(size_t)2 * p + 1])) continue;
                const double *T = &hyp[(size_t)12 * (pspan[(size_t)4 * p + 2] + b)];
                for (int k = 0; k < 9; k++) mR[(size_t)m * 9 + k] = T[k];
                for (int k = 0; k < 3; k++) mt[(size_t)m * 3 + k] = T[9 + k];
                has_mpose[(size_t)m] = 1;
                changed = true;
            }
        }
        return FID_OK;
    }

    // ---- Levenberg-Marquardt over the active observations of the placed markers in the posed views, from the poses held here, and the
    // records.  FID_E_INVALID_ARG with fid_last_error set: no view can be used, or fewer residuals than free parameters.
    fid_status solve(BldResult *res)
    {
        hipStream_t st = c->stream;
        std::vector<int> fin_slot((size_t)NI, -1), fin_id;  // the slots: the markers in the solve that have a pose, in id order
        for (int m = 0; m < NI; m++) {
            if (!placed[(size_t)m]) continue;
            if (!has_mpose[(size_t)m]) {
                mstatus[(size_t)m] = FID_BUILD_MARKER_NO_START;
                continue;
            }
            mstatus[(size_t)m] = fix_of[(size_t)m] >= 0 ? FID_BUILD_MARKER_FIXED : FID_BUILD_MARKER_SOLVED;
            fin_slot[(size_t)m] = (int)fin_id.size();
            fin_id.push_back(m);
        }
        const int FS = (int)fin_id.size();
        std::vector<int> voff((size_t)V, 0), vcnt((size_t)V, 0), omk, oslot, oview, mfree((size_t)FS + 1, -1), fslot;
        for (int s = 0; s < FS; s++)
            if (fix_of[(size_t)fin_id[(size_t)s]] < 0) {
                mfree[(size_t)s] = (int)fslot.size();
                fslot.push_back(s);
            }
        const int FM = (int)fslot.size(), n = 6 * FM;
        int n_used = 0;
        std::vector<std::vector<int>> slot_obs((size_t)FS);
        std::vector<uint32_t> links((size_t)FS * 4, 0u);
        for (int v = 0; v < V; v++) {
            voff[(size_t)v] = (int)omk.size();
            if (!has_vpose[(size_t)v] || !reached[(size_t)v]) {
                if (reached[(size_t)v] && vstatus[(size_t)v] != FID_BUILD_VIEW_NO_START) vstatus[(size_t)v] = FID_BUILD_VIEW_NO_START;
                continue;
            }
            for (size_t k = 0; k < kid[(size_t)v].size(); k++) {
                const int s = fin_slot[(size_t)kid[(size_t)v][k]];
                if (s < 0 || !active[(size_t)v][k]) continue;
                slot_obs[(size_t)s].push_back((int)omk.size());
                omk.push_back(v * pv + (int)k);
                oslot.push_back(s);
                oview.push_back(v);
            }
            vcnt[(size_t)v] = (int)omk.size() - voff[(size_t)v];
            if (vcnt[(size_t)v] > 0) {
                vstatus[(size_t)v] = FID_BUILD_VIEW_USED;
                n_used++;
                for (int a = voff[(size_t)v]; a < (int)omk.size(); a++)
                    for (int b = voff[(size_t)v]; b < (int)omk.size(); b++) links[(size_t)oslot[(size_t)a] * 4 + (oslot[(size_t)b] >> 5)] |= 1u << (oslot[(size_t)b] & 31);
            } else {
                vstatus[(size_t)v] = FID_BUILD_VIEW_NO_START;
            }
        }
        const int NO = (int)omk.size();
        const int n_free = 6 * FM + 6 * n_used;
        if (n_used == 0) return refuse("no view can be used (none has a start pose)"), FID_E_INVALID_ARG;
        if (8 * NO < n_free) return refuse(std::to_string(8 * NO) + " residuals for " + std::to_string(n_free) + " free parameters"), FID_E_INVALID_ARG;
        std::vector<int> moff((size_t)FS + 1, 0), mobs;
        for (int s = 0; s < FS; s++) {
            moff[(size_t)s] = (int)mobs.size();
            mobs.insert(mobs.end(), slot_obs[(size_t)s].begin(), slot_obs[(size_t)s].end());
        }
        moff[(size_t)FS] = (int)mobs.size();
        std::vector<double> mpar((size_t)FS * 6 + 6, 0.), mrt((size_t)FS * BLD_MR + BLD_MR, 0.), crt((size_t)FS * 12 + 12, 0.);
        for (int s = 0; s < FS; s++) {
            const int m = fin_id[(size_t)s];
            if (has_mrv[(size_t)m]) {  // (a solve's own parameters, not taken through the matrix and back)
                for (int k = 0; k < 3; k++) mpar[(size_t)s * 6 + k] = mrv[(size_t)m * 6 + k];
            } else {
                bld_rod_m2v(&mR[(size_t)m * 9], &mpar[(size_t)s * 6]);
            }
            for (int k = 0; k < 3; k++) mpar[(size_t)s * 6 + 3 + k] = mt[(size_t)m * 3 + k];
            for (int k = 0; k < 9; k++) mrt[(size_t)s * BLD_MR + k] = crt[(size_t)s * 12 + k] = mR[(size_t)m * 9 + k];
            for (int k = 0; k < 3; k++) mrt[(size_t)s * BLD_MR + 36 + k] = crt[(size_t)s * 12 + 9 + k] = mt[(size_t)m * 3 + k];
            mrt[(size_t)s * BLD_MR + 39] = (double)(float)(len[(size_t)m] / 2);
        }
        std::vector<fid_build_view> hv((size_t)V);
        memset(hv.data(), 0, sizeof(fid_build_view) * (size_t)V);
        for (int v = 0; v < V; v++) {
            hv[(size_t)v].status = vstatus[(size_t)v];
            hv[(size_t)v].n_over = n_over[(size_t)v];
        }
        BldCfg cfg = {};
        cfg.n_views = V;
        cfg.n_slots = FS;
        cfg.n_fm = FM;
        cfg.n = n;
        cfg.per_view = pv;
        cfg.max_iter = opts->max_iter;
        cfg.n_obs = NO;
        cfg.n_points = 4 * NO;
        cfg.n_views_used = n_used;
        cfg.n_free = n_free;
        cfg.eps = opts->eps;
        cfg.sigma_px = opts->sigma_px;
        BldState hs = {};
        hs.lambdaLg10 = -3;
        hs.needJ = 1;
        hs.done = opts->max_iter == 0 ? 1 : 0;
        hs.status = opts->max_iter == 0 ? FID_BUILD_MAX_ITER : FID_BUILD_OK;
        HIPCHK(c, hipMemcpyAsync(d_cfg, &cfg, sizeof(cfg), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_voff, voff.data(), sizeof(int) * V, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_vcnt, vcnt.data(), sizeof(int) * V, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_omk, omk.data(), sizeof(int) * NO, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_oslot, oslot.data(), sizeof(int) * NO, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_oview, oview.data(), sizeof(int) * NO, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_mobs, mobs.data(), sizeof(int) * NO, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_moff, moff.data(), sizeof(int) * (FS + 1), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_mfree, mfree.data(), sizeof(int) * (FS + 1), hipMemcpyHostToDevice, st));
        if (FM > 0) HIPCHK(c, hipMemcpyAsync(d_fslot, fslot.data(), sizeof(int) * FM, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_mpar, mpar.data(), sizeof(double) * 6 * FS, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_mcand, mpar.data(), sizeof(double) * 6 * FS, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_mrt, mrt.data(), sizeof(double) * BLD_MR * FS, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_crt, crt.data(), sizeof(double) * 12 * FS, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_vpose, vpose.data(), sizeof(double) * 6 * V, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_vout, hv.data(), sizeof(fid_build_view) * V, hipMemcpyHostToDevice, st));

        // ---- Levenberg-Marquardt: BLD_CHUNK trials, then the status
        const int model = pcam.model;
        auto system = [&](int final) {
            hipLaunchKernelGGL(k_build_prep, dim3(FS), dim3(64), 0, st, (const BldState *)d_state, (const int *)d_mfree, (const double *)d_mpar, d_mrt, final);
            // (the plumb-bob camera runs the rational instantiation: with k4 k5 k6 and s1 .. s4 zero -- PoseCam's D beyond the model's is zero --
            // its denominator is 1 and its prism terms are 0, so value and derivatives are the plumb-bob ones bit for bit; the plumb-bob
            // instantiation of this kernel is the one the compiler does not fit into 128 registers without spilling; k_build_eval runs the
            // same instantiation, and tests/test_gpu_map_build.py holds a plumb-bob call to the bytes of the rational call with zeros)
            POSE_CAM_DISPATCH(model == FID_CAM_PLUMB_BOB ? FID_CAM_RATIONAL : model,
                              if constexpr (CAM_MODEL != FID_CAM_PLUMB_BOB) hipLaunchKernelGGL(k_build_blocks<CAM_MODEL>, dim3(V), dim3(64), 0, st, (const BldState *)d_state, pcam, (const fid_marker *)d_mk,
                                                        (const int *)d_voff, (const int *)d_vcnt, (const int *)d_omk, (const int *)d_oslot, (const int *)d_mfree,
                                                        (const double *)d_mrt, (const double *)d_vpose, d_oblk, d_vblk, d_vcost, final));
            hipLaunchKernelGGL(k_build_schur, dim3(V), dim3(64), 0, st, (const BldState *)d_state, (const int *)d_voff, (const int *)d_vcnt, (const int *)d_oslot,
                               (const int *)d_mfree, (const double *)d_oblk, (const double *)d_vblk, d_ow, final);
        };
        auto factor = [&](int final) {
            if (FM == 0) return;
            hipLaunchKernelGGL(k_build_reduce, dim3(FM, FM), dim3(64), 0, st, (const BldCfg *)d_cfg, d_state, (const int *)d_fslot, (const int *)d_moff,
                               (const int *)d_mobs, (const int *)d_oview, (const double *)d_oblk, (const double *)d_ow, d_S, d_g, final);
            for (int k0 = 0; k0 < n; k0 += BLD_NB) {
                hipLaunchKernelGGL(k_build_panel, dim3((n - k0 + BLD_NB - 1) / BLD_NB), dim3(64), 0, st, (const BldCfg *)d_cfg, d_state, d_S, d_Dg, k0, final);
                const int T = (n - k0 - BLD_NB + BLD_NB - 1) / BLD_NB;
                if (T > 0) hipLaunchKernelGGL(k_build_update, dim3(T, T), dim3(256), 0, st, (const BldCfg *)d_cfg, (const BldState *)d_state, d_S, k0, final);
            }
        };
        int queued = 0;
        while (!hs.done) {
            for (int i = 0; i < BLD_CHUNK && queued < opts->max_iter; i++, queued++) {
                system(0);
                factor(0);
                hipLaunchKernelGGL(k_build_solve, dim3(1), dim3(256), 0, st, (const BldCfg *)d_cfg, d_state, (const double *)d_S, (const double *)d_Dg, (const double *)d_g,
                                   (const int *)d_mfree, (const double *)d_mpar, (const int *)d_vcnt, (const double *)d_vcost, d_dx, d_mcand, d_crt);
                POSE_CAM_DISPATCH(model == FID_CAM_PLUMB_BOB ? FID_CAM_RATIONAL : model,  // (the blocks kernel's instantiation: the two costs of a trial come from one code)
                                  if constexpr (CAM_MODEL != FID_CAM_PLUMB_BOB) hipLaunchKernelGGL(k_build_eval<CAM_MODEL>, dim3(V), dim3(64), 0, st, (const BldState *)d_state, pcam,
                                                            (const fid_marker *)d_mk, (const int *)d_voff, (const int *)d_vcnt, (const int *)d_omk,
                                                            (const int *)d_oslot, (const int *)d_mfree, (const double *)d_mrt, (const double *)d_crt,
                                                            (const double *)d_vpose, (const double *)d_oblk, (const double *)d_vblk, (const double *)d_dx, d_vcand,
                                                            d_vccost, d_dnpn));
                hipLaunchKernelGGL(k_build_accept, dim3(1), dim3(256), 0, st, (const BldCfg *)d_cfg, d_state, (const int *)d_vcnt, (const int *)d_mfree, d_vpose,
                                   (const double *)d_vcand, (const double *)d_vccost, (const double *)d_dnpn, d_mpar, (const double *)d_mcand);
            }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&hs.lambdaLg10, &d_state->lambdaLg10, sizeof(int) * 4, hipMemcpyDeviceToHost, st));  // lambdaLg10 trials status done
            HIPCHK(c, hipStreamSynchronize(st));
            if (!hs.done && queued >= opts->max_iter) {
                c->last_error = std::string(who) + ": the device did not report the stop after max_iter trials";
                return FID_E_HIP;
            }
        }
        system(1);
        hipLaunchKernelGGL(k_build_finish, dim3(1), dim3(256), 0, st, (const BldCfg *)d_cfg, d_state, (const int *)d_vcnt, (const double *)d_vcost,
                           (const double *)d_vpose, d_out, d_vout);
        factor(1);
        hipLaunchKernelGGL(k_build_cov, dim3(FS), dim3(256), 0, st, (const BldCfg *)d_cfg, (const BldState *)d_state, (const double *)d_S, (const double *)d_Dg, (const int *)d_mfree,
                           (const int *)d_moff, (const int *)d_mobs, (const double *)d_oblk, d_mout);
        HIPCHK(c, hipGetLastError());
        std::vector<double> mout((size_t)FS * 40);
        HIPCHK(c, hipMemcpyAsync(&res->out, d_out, sizeof(fid_build_out), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(hv.data(), d_vout, sizeof(fid_build_view) * (size_t)V, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(mout.data(), d_mout, sizeof(double) * 40 * (size_t)FS, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(mpar.data(), d_mpar, sizeof(double) * 6 * (size_t)FS, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        // ---- the records, and the poses this solve leaves to the next one
        res->views = hv;
        res->n_obs = NO;
        res->active = active;
        res->markers.assign((size_t)NI, fid_build_marker());
        for (int m = 0; m < NI; m++) {
            fid_build_marker &o = res->markers[(size_t)m];
            memset(&o, 0, sizeof(o));
            o.id = ids[(size_t)m];
            o.status = mstatus[(size_t)m];
            o.n_views = nview[(size_t)m];
            o.slot = fin_slot[(size_t)m];
            o.entry.id = o.id;
            o.entry.len = len[(size_t)m];
            const int s = o.slot;
            if (s < 0) continue;
            for (int k = 0; k < 4; k++) o.links[k] = links[(size_t)s * 4 + k];
            o.rms = mout[(size_t)s * 40 + 36];
            if (fix_of[(size_t)m] >= 0) {
                o.entry = fixed[fix_of[(size_t)m]];
            } else {
                bld_rod_v2m(&mpar[(size_t)s * 6], o.entry.R);
                for (int k = 0; k < 3; k++) o.entry.t[k] = mpar[(size_t)s * 6 + 3 + k];
                for (int k = 0; k < 36; k++) o.cov[k] = mout[(size_t)s * 40 + k];
                has_mrv[(size_t)m] = 1;
                for (int k = 0; k < 6; k++) mrv[(size_t)m * 6 + k] = mpar[(size_t)s * 6 + k];
                for (int k = 0; k < 9; k++) mR[(size_t)m * 9 + k] = o.entry.R[k];
                for (int k = 0; k < 3; k++) mt[(size_t)m * 3 + k] = o.entry.t[k];
            }
        }
        for (int v = 0; v < V; v++)
            if (hv[(size_t)v].status == FID_BUILD_VIEW_USED)
                for (int i = 0; i < 3; i++) {
                    vpose[(size_t)v * 6 + i] = hv[(size_t)v].rvec[i];
                    vpose[(size_t)v * 6 + 3 + i] = hv[(size_t)v].tvec[i];
                }
        return FID_OK;
    }

    // ---- err of every kept observation whose view and marker have a pose, under the poses held here (k_build_obs_err)
    fid_status obs_err(std::vector<std::vector<double>> *err)
    {
        hipStream_t st = c->stream;
        if (evoff.empty()) {  // the list: once, the start being over
            evoff.assign((size_t)V, 0);
            evcnt.assign((size_t)V, 0);
            std::vector<int> eomk, eom;
            for (int v = 0; v < V; v++) {
                evoff[(size_t)v] = (int)eomk.size();
                if (!has_vpose[(size_t)v]) continue;
                for (size_t k = 0; k < kid[(size_t)v].size(); k++) {
                    if (!has_mpose[(size_t)kid[(size_t)v][k]]) continue;
                    eomk.push_back(v * pv + (int)k);
                    eom.push_back(kid[(size_t)v][k]);
                }
                evcnt[(size_t)v] = (int)eomk.size() - evoff[(size_t)v];
            }
            n_err = (int)eomk.size();
            HIPCHK(c, hipMemcpyAsync(d_evoff, evoff.data(), sizeof(int) * V, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_evcnt, evcnt.data(), sizeof(int) * V, hipMemcpyHostToDevice, st));
            if (n_err > 0) {
                HIPCHK(c, hipMemcpyAsync(d_eomk, eomk.data(), sizeof(int) * n_err, hipMemcpyHostToDevice, st));
                HIPCHK(c, hipMemcpyAsync(d_eom, eom.data(), sizeof(int) * n_err, hipMemcpyHostToDevice, st));
            }
            HIPCHK(c, hipStreamSynchronize(st));  // (eomk and eom leave scope)
        }
        std::vector<double> emrt((size_t)NI * 16, 0.);
        for (int m = 0; m < NI; m++) {
            for (int k = 0; k < 9; k++) emrt[(size_t)m * 16 + k] = mR[(size_t)m * 9 + k];
            for (int k = 0; k < 3; k++) emrt[(size_t)m * 16 + 9 + k] = mt[(size_t)m * 3 + k];
            emrt[(size_t)m * 16 + 12] = (double)(float)(len[(size_t)m] / 2);
        }
        std::vector<double> herr((size_t)std::max(n_err, 1), -1.);
        HIPCHK(c, hipMemcpyAsync(d_emrt, emrt.data(), sizeof(double) * 16 * (size_t)NI, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_evpose, vpose.data(), sizeof(double) * 6 * (size_t)V, hipMemcpyHostToDevice, st));
        POSE_CAM_DISPATCH(pcam.model, hipLaunchKernelGGL(k_build_obs_err<CAM_MODEL>, dim3(V), dim3(64), 0, st, pcam, (const fid_marker *)d_mk, (const int *)d_evoff,
                                                         (const int *)d_evcnt, (const int *)d_eomk, (const int *)d_eom, (const double *)d_emrt, (const double *)d_evpose,
                                                         d_err));
        HIPCHK(c, hipGetLastError());
        if (n_err > 0) HIPCHK(c, hipMemcpyAsync(herr.data(), d_err, sizeof(double) * (size_t)n_err, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        err->assign((size_t)V, {});
        for (int v = 0; v < V; v++) {
            (*err)[(size_t)v].assign(kid[(size_t)v].size(), -1.);
            if (!has_vpose[(size_t)v]) continue;
            int o = evoff[(size_t)v];
            for (size_t k = 0; k < kid[(size_t)v].size(); k++)
                if (has_mpose[(size_t)kid[(size_t)v][k]]) (*err)[(size_t)v][k] = herr[(size_t)o++];
        }
        return FID_OK;
    }
};

void bld_write(const BldResult &r, fid_build_out *out, fid_build_marker *markers_out, fid_build_view *views)
{
    *out = r.out;
    if (views) memcpy(views, r.views.data(), sizeof(fid_build_view) * r.views.size());
    if (!r.markers.empty()) memcpy(markers_out, r.markers.data(), sizeof(fid_build_marker) * r.markers.size());
}

}  // namespace

fid_status fid_build_map_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, const int32_t *n_per_view, int32_t n_views, int32_t cap_per_view,
                             const fid_map_entry *fixed, int32_t n_fixed, const fid_build_opts *opts, fid_build_out *out, fid_build_marker *markers_out,
                             int32_t cap_markers, int32_t *n_markers_out, fid_build_view *views)
{
    if (!c) return FID_E_INVALID_ARG;
    BldRun r = {};
    r.c = c, r.who = "fid_build_map_cam", r.markers = markers, r.n_per_view = n_per_view, r.V = n_views, r.cap_per_view = cap_per_view, r.fixed = fixed,
    r.n_fixed = n_fixed, r.opts = opts;
    fid_status rc = r.check(camera, out, markers_out, cap_markers, n_markers_out);
    if (rc == FID_OK) rc = r.select(cap_markers, n_markers_out);
    if (rc != FID_OK) return rc;
    const bool any = r.plan();
    if (r.n_in > FID_BUILD_MAX_MARKERS)
        return r.refuse(std::to_string(r.n_in) + " markers enter the solve, at most " + std::to_string(FID_BUILD_MAX_MARKERS) + " (FID_BUILD_MAX_MARKERS) can"),
               FID_E_UNSUPPORTED;
    if (!any) return r.refuse("no view holds a fixed fiducial"), FID_E_INVALID_ARG;
    BldResult res;
    if ((rc = r.alloc()) != FID_OK || (rc = r.stage()) != FID_OK || (rc = r.start_plain()) != FID_OK || (rc = r.solve(&res)) != FID_OK) return rc;
    bld_write(res, out, markers_out, views);
    return FID_OK;
}

fid_status fid_build_map_robust_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, const int32_t *n_per_view, int32_t n_views,
                                    int32_t cap_per_view, const fid_map_entry *fixed, int32_t n_fixed, const fid_build_opts *opts,
                                    const fid_build_robust_opts *ropts, fid_build_out *out, fid_build_robust_out *robust_out, fid_build_marker *markers_out,
                                    int32_t cap_markers, int32_t *n_markers_out, fid_build_view *views, uint8_t *obs_state, double *obs_err_px,
                                    int32_t *marker_outliers, int32_t *view_outliers)
{
    if (!c) return FID_E_INVALID_ARG;
    BldRun r = {};
    r.c = c, r.who = "fid_build_map_robust_cam", r.markers = markers, r.n_per_view = n_per_view, r.V = n_views, r.cap_per_view = cap_per_view, r.fixed = fixed,
    r.n_fixed = n_fixed, r.opts = opts, r.robust = true;
    if (n_markers_out) *n_markers_out = 0;
    if (!ropts || !robust_out) return r.refuse("a NULL pointer"), FID_E_INVALID_ARG;
    if (!(ropts->inlier_px > 0.) || !bld_finite(ropts->inlier_px) || ropts->min_views_place < 1)
        return r.refuse("inlier_px must be finite and > 0, min_views_place >= 1"), FID_E_INVALID_ARG;
    fid_status rc = r.check(camera, out, markers_out, cap_markers, n_markers_out);
    if (rc == FID_OK) rc = r.select(cap_markers, n_markers_out);
    if (rc != FID_OK) return rc;
    const bool any = r.plan();
    if (r.n_in > FID_BUILD_MAX_MARKERS)
        return r.refuse(std::to_string(r.n_in) + " markers enter the solve, at most " + std::to_string(FID_BUILD_MAX_MARKERS) + " (FID_BUILD_MAX_MARKERS) can"),
               FID_E_UNSUPPORTED;
    if (!any) return r.refuse("no view holds a fixed fiducial"), FID_E_INVALID_ARG;
    if ((rc = r.alloc()) != FID_OK || (rc = r.stage()) != FID_OK || (rc = r.start_robust(*ropts)) != FID_OK) return rc;
    const int V = n_views;
    BldResult fin, cur;
    int rounds = 0, stable = 0, n_obs0 = 0;
    {  // the first set: what the start admits within inlier_px
        std::vector<std::vector<double>> e0;
        if ((rc = r.obs_err(&e0)) != FID_OK) return rc;
        const double thr0 = ropts->inlier_px;
        for (int v = 0; v < V; v++)
            for (size_t k = 0; k < e0[(size_t)v].size(); k++)
                if (e0[(size_t)v][k] >= 0. || e0[(size_t)v][k] != e0[(size_t)v][k]) r.active[(size_t)v][k] = e0[(size_t)v][k] <= thr0 ? 1 : 0;
        if (!r.plan()) return r.refuse("no view holds a fixed fiducial within inlier_px of the start"), FID_E_INVALID_ARG;
    }
    for (int round = 0; round < FID_BUILD_ROBUST_SOLVES; round++) {
        if (round > 0) HIPCHK(c, hipMemsetAsync(r.M + r.off_solve0, 0, r.off_solve1 - r.off_solve0, c->stream));  // (a solve starts from the buffer a call starts from)
        const std::string error_before = c->last_error;
        rc = r.solve(&cur);
        if (rc == FID_E_INVALID_ARG && round > 0) {  // (too little is left after trimming: the round before stands, stable = 0)
            c->last_error = error_before;  // (the call succeeds: the refusal's text is not its)
            break;
        }
        if (rc != FID_OK) return rc;
        if ((rc = r.obs_err(&cur.err)) != FID_OK) return rc;
        fin = cur;
        rounds = round + 1;
        n_obs0 = r.n_err;
        std::vector<std::vector<char>> next = r.active;
        for (int v = 0; v < V; v++)
            for (size_t k = 0; k < next[(size_t)v].size(); k++)
                if (cur.err[(size_t)v][k] >= 0. || cur.err[(size_t)v][k] != cur.err[(size_t)v][k]) next[(size_t)v][k] = cur.err[(size_t)v][k] <= ropts->inlier_px ? 1 : 0;
        if (next == r.active) {
            stable = 1;
            break;
        }
        if (round + 1 == FID_BUILD_ROBUST_SOLVES) break;
        r.active = next;
        if (!r.plan()) break;  // (no reached view is left)
    }
    bld_write(fin, out, markers_out, views);
    fid_build_robust_out ro = {};
    ro.rounds = rounds;
    ro.stable = stable;
    ro.n_obs = n_obs0;
    ro.worst_inlier_px = ro.best_outlier_px = -1.;
    if (obs_state) memset(obs_state, FID_BUILD_OBS_NOT_KEPT, (size_t)V * cap_per_view);
    if (obs_err_px)
        for (size_t i = 0; i < (size_t)V * cap_per_view; i++) obs_err_px[i] = -1.;
    if (marker_outliers)
        for (int m = 0; m < cap_markers; m++) marker_outliers[m] = 0;
    if (view_outliers)
        for (int v = 0; v < V; v++) view_outliers[v] = 0;
    for (int v = 0; v < V; v++)
        for (size_t k = 0; k < r.kid[(size_t)v].size(); k++) {
            const int m = r.kid[(size_t)v][k];
            const size_t at = (size_t)v * cap_per_view + r.kept[(size_t)v][k];
            const double e = fin.err[(size_t)v][k];
            const int ms = fin.markers[(size_t)m].status;
            int state = FID_BUILD_OBS_LEFT_OUT;
            if (!fin.active[(size_t)v][k]) {
                state = FID_BUILD_OBS_OUTLIER;
                ro.n_outliers++;
                if (e >= 0. && (ro.best_outlier_px < 0. || e < ro.best_outlier_px)) ro.best_outlier_px = e;
                if (marker_outliers) marker_outliers[m]++;
                if (view_outliers) view_outliers[v]++;
            } else if ((ms == FID_BUILD_MARKER_FIXED || ms == FID_BUILD_MARKER_SOLVED) && fin.views[(size_t)v].status == FID_BUILD_VIEW_USED) {
                state = FID_BUILD_OBS_INLIER;
                ro.n_inliers++;
                if (!(e <= ro.worst_inlier_px)) ro.worst_inlier_px = e;
            }
            if (obs_state) obs_state[at] = (uint8_t)state;
            if (obs_err_px) obs_err_px[at] = e >= 0. ? e : -1.;
        }
    *robust_out = ro;
    return FID_OK;
}

fid_status fid_map_save_file(const char *path, const fid_build_marker *markers, int32_t n)
{
    g_map_error.clear();
    if (!path || n < 0 || (n > 0 && !markers)) {
        g_map_error = "a NULL pointer or a negative count";
        return FID_E_INVALID_ARG;
    }
    FILE *fp = fopen(path, "w");
    if (!fp) {
        g_map_error = std::string("cannot open ") + path + " for writing";
        return FID_E_INVALID_ARG;
    }
    const double r2d = 180.0 / 3.14159265358979323846;
    for (int i = 0; i < n; i++) {
        const fid_build_marker &m = markers[i];
        if (m.status != FID_BUILD_MARKER_FIXED && m.status != FID_BUILD_MARKER_SOLVED) continue;
        const double *R = m.entry.R;
        double roll, pitch, yaw;
        if (fabs(R[6]) >= 1.) {  // (the gimbal lock: yaw = 0 takes the whole rotation about the vertical)
            yaw = 0.;
            pitch = R[6] < 0. ? 1.57079632679489661923 : -1.57079632679489661923;
            roll = R[6] < 0. ? atan2(R[1], R[2]) : atan2(-R[1], -R[2]);
        } else {
            pitch = asin(-R[6]);
            roll = atan2(R[7], R[8]);
            yaw = atan2(R[3], R[0]);
        }
        const double var = m.status == FID_BUILD_MARKER_SOLVED ? (m.cov[21] + m.cov[28] + m.cov[35]) / 3. : 0.;
        fprintf(fp, "%d %lf %lf %lf %lf %lf %lf %lf %d", m.id, m.entry.t[0], m.entry.t[1], m.entry.t[2], roll * r2d, pitch * r2d, yaw * r2d, var, m.n_views);
        std::vector<int> linked;
        for (int k = 0; k < n; k++) {
            const fid_build_marker &o = markers[k];
            if (k == i || o.slot < 0 || o.slot >= 128 || (o.status != FID_BUILD_MARKER_FIXED && o.status != FID_BUILD_MARKER_SOLVED)) continue;
            if (m.links[o.slot >> 5] >> (o.slot & 31) & 1u) linked.push_back(o.id);
        }
        std::sort(linked.begin(), linked.end());
        for (int id : linked) fprintf(fp, " %d", id);
        fprintf(fp, "\n");
    }
    if (fclose(fp) != 0) {
        g_map_error = std::string("cannot write ") + path;
        return FID_E_INVALID_ARG;
    }
    return FID_OK;
}
