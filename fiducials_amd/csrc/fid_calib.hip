// fid_calib.hip -- camera calibration from views of the map (fid_abi.h: "camera calibration from views of the map").  Part of the
// fid_api.hip translation unit, behind fid_map_pose_robust.hip.  The gather, the planarity test, the DLT and the start poses are
// k_map_pose's (fid_map_pose.hip); rodrigues_v2m's derivative, solve6_spd and CvLevMarq's damping table come from fid_pnp.h; the
// residual function in the restatement's arithmetic (cal_rotation_value, cal_pinhole, cal_distort, cal_project) and its derivatives
// with respect to the pose, fx fy cx cy and every distortion coefficient (cal_row) are in fid_cal_model.h, shared with fid_map_build.hip.
//
// The normal matrix of the joint problem is an arrowhead: the n x n block A of the free intrinsics (n <= 16), one 6 x 6 block C_v per
// view and the n x 6 couplings B_v.  One trial step of Levenberg-Marquardt is four launches on the context's stream:
//   K22 k_calib_blocks   a wave per view.  With new parameters: the residuals and Jacobian rows of the view, 64 at a time -- a lane
//                        computes one row (16 intrinsics columns, 6 pose columns, the residual) and puts it in LDS; then every lane
//                        adds, row by row, the products of ITS entries of the upper triangle of [J e]^T [J e] (at most 276 entries,
//                        five per lane): each entry is one serial sum in residual order, no lane holds more than five partial sums,
//                        and nothing is reduced across lanes.  The view's cost is the per-lane sum of the lane's squared residuals
//                        and a butterfly (k_calib_eval's order and expressions, so that the two agree to the bit).  Always: the view's Schur pieces
//                        under the current damping, W = B (C + lambda diag C)^-1 by solve6_spd on lane j for row j, then W B^T and
//                        W g_pose.
//   K23 k_calib_solve    one workgroup.  Thread (j, k) adds A_v[j][k] and the Schur pieces over the views in index order; one wave
//                        factors the reduced n x n matrix (Cholesky in LDS, a lane per row) and solves for the intrinsics' step.
//   K24 k_calib_eval     a wave per view: the view's pose step by back-substitution, the candidate pose, the cost there.
//   K25 k_calib_accept   one wave: the candidate's cost over the views in index order, CvLevMarq's accept / reject, the stop.
// Every kernel of a trial returns at once when the stop has been reached, so the host queues CAL_CHUNK trials between two reads of
// the 16-byte status (DESIGN section "calibration" has both ways of driving the loop measured).  After the stop: k_calib_blocks and
// k_calib_solve once more with FINAL, undamped, at the returned parameters: the cost, the inverse of the Schur complement, std_dev,
// the per-view records.
//   K21 k_calib_start    a wave per view, once: the gather (k_map_pose's stage (1)) -> the used markers' list positions and map entries
//                        for the other kernels; with START_AUTO the planarity test, the DLT homography to the float pixels and the
//                        view's two focal constraints.  (The host adds the constraints in view order -- a 2 x 2 system -- because it
//                        needs the start camera by value for k_map_pose's launch anyway.)
//       k_calib_init     one wave, once: which views are used, their start poses from k_map_pose's records, the counts.
// No kernel keeps an array that is indexed at run time in registers: rows, triangles and factors live in LDS.  No scratch, no spills
// (tests/test_calib_kernel_allocations.py).
// K22 and K24 are thin: their bodies are the device functions cal_view_blocks and cal_view_eval over a row source (CalMarkers here),
// and k_calib_init's is cal_init_views over the start-pose record.  fid_calib_points.hip instantiates the same bodies over a per-view
// point table for fid_calibrate_charuco, and both entry points share the host steps at the end of this file.

#define CAL_COLS 23   // a Jacobian row in LDS: 16 intrinsics slots, 6 pose parameters, the residual
#define CAL_TRI 276   // the upper triangle of 23 x 23
#define CAL_SCH 272   // W B^T as 16 x 16, then W g_pose (16)
#ifndef CAL_CHUNK
#define CAL_CHUNK 8   // trials queued between two reads of the status
#endif

struct CalCfg {
    int nI;            // free intrinsics
    int col[16];       // the slot of free intrinsic j, ascending
    int fix_aspect;    // fx = aspect * fy, fy's slot is free
    int start_auto, min_markers, max_iter, n_views, per_view;
    int per_item;      // image points an item of a view's list brings: 4 (a marker), 1 (a point of fid_calib_points.hip)
    double aspect, eps;
};
struct CalState {
    double k[16], cand[16];  // the slots fx fy cx cy D[0..11]: current and candidate
    double dI[16];           // the trial step of the free intrinsics
    double cost, start_cost, dnI, pnI;
    int lambdaLg10, trials, status, done, needJ, bad, n_views_used, n_points;
};

#include "fid_cal_model.h"

// cvInitIntrinsicParams2D's two rows for a view from its homography h (changed in place): c6 = {a, b, c} of a X + b Y = c, twice.
// -> whether all six are finite
__device__ __forceinline__ bool cal_focal_rows(double h[9], double cx0, double cy0, double c6[6])
{
    for (int j = 0; j < 3; j++) {
        h[j] -= h[6 + j] * cx0;
        h[3 + j] -= h[6 + j] * cy0;
    }
    double h1[3], h2[3], d1[3], d2[3], n4[4] = {0, 0, 0, 0};
    for (int j = 0; j < 3; j++) {
        const double t0 = h[3 * j], t1 = h[3 * j + 1];
        h1[j] = t0;
        h2[j] = t1;
        d1[j] = (t0 + t1) * 0.5;
        d2[j] = (t0 - t1) * 0.5;
        n4[0] += t0 * t0; n4[1] += t1 * t1; n4[2] += d1[j] * d1[j]; n4[3] += d2[j] * d2[j];
    }
    for (int j = 0; j < 4; j++) n4[j] = 1. / sqrt(n4[j]);
    for (int j = 0; j < 3; j++) {
        h1[j] *= n4[0]; h2[j] *= n4[1]; d1[j] *= n4[2]; d2[j] *= n4[3];
    }
    c6[0] = h1[0] * h2[0]; c6[1] = h1[1] * h2[1]; c6[2] = -h1[2] * h2[2];
    c6[3] = d1[0] * d2[0]; c6[4] = d1[1] * d2[1]; c6[5] = -d1[2] * d2[2];
    bool fin = true;
    for (int j = 0; j < 6; j++) fin = fin && c6[j] - c6[j] == 0.;
    return fin;
}

// ------------------------------------------------------------------------------------------------ K21: the views' used markers
// vinfo[4 v + ..]: 0 n_used, 1 n_over, 2 the view's status (k_calib_init), 3 bit 0: coplanar, bit 1: the homography exists.
// con[6 v + ..]: the two focal constraints a X + b Y = c of the view.
// (the upper bounds of the two workgroup sizes below are never launched: they keep the descriptor's register allocation at what the
// kernel uses instead of the floor its static LDS would allow, fid_kernels.hip WALKER_WG_ATTR)
__global__ WALKER_WG_ATTR(64, 1024) void k_calib_start(const fid_marker *__restrict__ markers, const int *__restrict__ n_per_view, int per_view,
                                                     const int *__restrict__ map_ids, const double *__restrict__ map_obj, int map_n, int want_auto,
                                                     double cx0, double cy0, int2 *__restrict__ sel, int *__restrict__ vinfo, double *__restrict__ con)
{
    __shared__ MpLds s;
    const int v = blockIdx.x, lane = threadIdx.x;
    const fid_marker *mlist = markers + (long long)v * per_view;
    int nm = n_per_view[v];
    nm = nm < 0 ? 0 : (nm > per_view ? per_view : nm);
    map_n = map_n > FID_MAP_MAX_ENTRIES ? FID_MAP_MAX_ENTRIES : map_n;
    // ---- k_map_pose's stage (1)
    for (int e = lane; e < MP_BIT_WORDS; e += 64) s.seen[e] = s.dup[e] = 0u;
    SR_LDS_SYNC();
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        const int idx = m < nm ? mp_find(map_ids, map_n, mlist[m].id) : -1;
        if (idx >= 0) {
            const unsigned bit = 1u << (idx & 31);
            if (atomicOr(&s.seen[idx >> 5], bit) & bit) atomicOr(&s.dup[idx >> 5], bit);
        }
    }
    SR_LDS_SYNC();
    int found = 0;
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        int idx = m < nm ? mp_find(map_ids, map_n, mlist[m].id) : -1;
        if (idx >= 0 && (s.dup[idx >> 5] >> (idx & 31) & 1u)) idx = -1;
        const unsigned long long hit = __ballot(idx >= 0);
        if (idx >= 0) {
            const int pos = found + __builtin_popcountll(hit & ((1ull << lane) - 1ull));
            if (pos < MP_MAX_USED) {
                s.mk[pos] = m;
                s.ent[pos] = idx;
            }
        }
        found += __builtin_popcountll(hit);
    }
    const int n_over = found > MP_MAX_USED ? found - MP_MAX_USED : 0;
    found -= n_over;
    SR_LDS_SYNC();
    for (int k = lane; k < found; k += 64) sel[(size_t)v * MP_MAX_USED + k] = make_int2(s.mk[k], s.ent[k]);
    int flags = 0;
    double c6[6] = {0, 0, 0, 0, 0, 0};
    if (want_auto && found > 0) {
        const int npts = 4 * found;
        for (int p = lane; p < npts; p += 64) {
            const int k = p >> 2, q = p & 3;
            const fid_marker *mk = mlist + s.mk[k];
            const double *src = map_obj + (size_t)s.ent[k] * 12 + q * 3;
            for (int a = 0; a < 3; a++) s.obj[p][a] = src[a];
            s.mn[p][0] = mk->corners[2 * q];  // (findHomography's input is float: the corners as they are)
            s.mn[p][1] = mk->corners[2 * q + 1];
        }
        SR_LDS_SYNC();
        // ---- k_map_pose's stage (2)
        double Mc[3] = {0, 0, 0}, W[3], Vt[3][3];
        for (int p = lane; p < npts; p += 64)
            for (int a = 0; a < 3; a++) Mc[a] += s.obj[p][a];
        for (int a = 0; a < 3; a++) Mc[a] = wave_sum_f64(Mc[a]) / npts;
        double m6[6] = {0, 0, 0, 0, 0, 0};
        for (int p = lane; p < npts; p += 64) {
            const double d[3] = {s.obj[p][0] - Mc[0], s.obj[p][1] - Mc[1], s.obj[p][2] - Mc[2]};
            m6[0] += d[0] * d[0]; m6[1] += d[0] * d[1]; m6[2] += d[0] * d[2];
            m6[3] += d[1] * d[1]; m6[4] += d[1] * d[2]; m6[5] += d[2] * d[2];
        }
        for (int i = 0; i < 6; i++) m6[i] = wave_sum_f64(m6[i]);
        double MM[3][3] = {{m6[0], m6[1], m6[2]}, {m6[1], m6[3], m6[4]}, {m6[2], m6[4], m6[5]}};
        pnp_scatter_eig(MM, W, Vt);
        if (W[2] / W[1] < 1e-3) {
            flags |= 1;
            double Rt[9], tt[3], h[9];
            pnp_plane_frame(Vt, Mc, Rt, tt);
            for (int p = lane; p < npts; p += 64) {
                const double *src = s.obj[p];
                s.Mxy[p][0] = (float)(Rt[0] * src[0] + Rt[1] * src[1] + Rt[2] * src[2] + tt[0]);
                s.Mxy[p][1] = (float)(Rt[3] * src[0] + Rt[4] * src[1] + Rt[5] * src[2] + tt[1]);
            }
            SR_LDS_SYNC();
            if (pnp_homography_dlt(MpView{&s, found}, npts, lane, h) && cal_focal_rows(h, cx0, cy0, c6)) flags |= 2;
        }
    }
    if (lane == 0) {
        vinfo[4 * v] = found;
        vinfo[4 * v + 1] = n_over;
        vinfo[4 * v + 2] = 0;
        vinfo[4 * v + 3] = flags;
        for (int j = 0; j < 6; j++) con[6 * v + j] = c6[j];
    }
}

// which views are used, their start poses, the counts (one wave).  REC: fid_map_pose_out or fid_charuco_pose_out, the record of the
// view's start pose; posed(record) says whether it holds one.
template <class REC, class POSED>
__device__ __forceinline__ void cal_init_views(const CalCfg *__restrict__ cfg, CalState *__restrict__ st, int *__restrict__ vinfo,
                                               const REC *__restrict__ vpose, double *__restrict__ pose, POSED posed)
{
    const int lane = threadIdx.x;
    int nv = 0, np = 0;
    for (int v = lane; v < cfg->n_views; v += 64) {
        const int n_used = vinfo[4 * v];
        int status = FID_CALIB_VIEW_USED;
        if (n_used < cfg->min_markers || n_used < 1) {
            status = FID_CALIB_VIEW_FEW;
        } else {
            const REC *o = vpose + v;
            bool ok = posed(o);
            for (int i = 0; i < 3; i++) ok = ok && o->rvec[i] - o->rvec[i] == 0. && o->tvec[i] - o->tvec[i] == 0.;
            if (cfg->start_auto && !(vinfo[4 * v + 3] & 2)) ok = false;
            if (!ok) status = FID_CALIB_VIEW_NO_START;
            for (int i = 0; i < 3; i++) {
                pose[6 * v + i] = ok ? o->rvec[i] : 0.;
                pose[6 * v + 3 + i] = ok ? o->tvec[i] : 0.;
            }
        }
        vinfo[4 * v + 2] = status;
        if (status == FID_CALIB_VIEW_USED) {
            nv++;
            np += cfg->per_item * n_used;
        }
    }
    for (int m = 1; m < 64; m <<= 1) {
        nv += __shfl_xor(nv, m, WAVE);
        np += __shfl_xor(np, m, WAVE);
    }
    if (lane == 0) {
        st->n_views_used = nv;
        st->n_points = np;
    }
}

__global__ __launch_bounds__(64) void k_calib_init(const CalCfg *__restrict__ cfg, CalState *__restrict__ st, int *__restrict__ vinfo,
                                                    const fid_map_pose_out *__restrict__ vpose, double *__restrict__ pose)
{
    cal_init_views(cfg, st, vinfo, vpose, pose, [](const fid_map_pose_out *o) { return o->n_markers > 0 && o->image_error >= 0.; });
}

// ------------------------------------------------------------------------------------------------ where a view's residuals come from
// The bodies of the per-view kernels K22 and K24 are written over a source SRC: bind(v, cfg) turns to view v, residual r of
// the view (r < PER_ITEM * 2 * n_used) has the object point object(r, M) and the image coordinate image(r).
// CalMarkers: the used markers' list positions and map entries (k_calib_start) -- residual r is coordinate r & 1 of corner (r >> 1) & 3
// of used marker r >> 3.  The point route's source is CalPoints (fid_calib_points.hip).
struct CalMarkers {
    static constexpr int PER_ITEM = 4;
    const fid_marker *__restrict__ markers;
    const int2 *__restrict__ sel;
    const double *__restrict__ map_obj;
    const fid_marker *mlist;
    const int2 *vs;
    __device__ __forceinline__ void bind(int v, const CalCfg *__restrict__ cfg)
    {
        mlist = markers + (long long)v * cfg->per_view;
        vs = sel + (size_t)v * MP_MAX_USED;
    }
    __device__ __forceinline__ void object(int r, double M[3]) const
    {
        const int p = r >> 1, k = p >> 2, q = p & 3;
        const double *src = map_obj + (size_t)vs[k].y * 12 + q * 3;
        M[0] = src[0];
        M[1] = src[1];
        M[2] = src[2];
    }
    __device__ __forceinline__ double image(int r) const
    {
        const int p = r >> 1, su = r & 1, k = p >> 2, q = p & 3;
        return (double)mlist[vs[k].x].corners[2 * q + su];
    }
};

// ------------------------------------------------------------------------------------------------ K22: a view's blocks
// blk[CAL_TRI v + ..]: the packed upper triangle of [J e]^T [J e] over the view's residuals, J's columns the free intrinsics (cfg->col's
// order) and then the view's pose, N = nI + 7 columns with the residual.  sch[CAL_SCH v + ..]: W B^T (16 j + k) and W g_pose (256 + j).
template <int MODEL, class SRC>
__device__ __forceinline__ void cal_view_blocks(const CalCfg *__restrict__ cfg, const CalState *__restrict__ st, SRC src, const int *__restrict__ vinfo,
                                                const double *__restrict__ pose, double *__restrict__ blk, double *__restrict__ sch,
                                                double *__restrict__ cost, int final)
{
    __shared__ double rows[64][CAL_COLS];
    __shared__ double tri[CAL_TRI];
    __shared__ double rot[36], rtmp[80];
    const int v = blockIdx.x, lane = threadIdx.x;
    if (!final && st->done) return;
    if (vinfo[4 * v + 2] != FID_CALIB_VIEW_USED) return;
    const int nI = cfg->nI, N = nI + 7, nent = N * (N + 1) / 2;
    if (final || st->needJ) {
        cal_rotation_lds(pose + 6 * v, rot, rtmp, lane);  // (first, while nothing else is held in registers)
        // the two columns of this lane's entries e = lane, lane + 64, ... (entry e of the triangle -> (a, b) -> their columns in a row)
        int ca[5], cb[5];
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const int e = lane + 64 * q;
            int a = 0, r = e < nent ? e : 0;
            while (r >= N - a) {
                r -= N - a;
                a++;
            }
            const int b = a + r;
            ca[q] = a < nI ? cfg->col[a] : 16 + (a - nI);
            cb[q] = b < nI ? cfg->col[b] : 16 + (b - nI);
        }
        double K[9] = {st->k[0], 0., st->k[2], 0., st->k[1], st->k[3], 0., 0., 1.}, kd[12], tv[3];
#pragma unroll
        for (int i = 0; i < 12; i++) kd[i] = st->k[4 + i];
#pragma unroll
        for (int i = 0; i < 3; i++) tv[i] = pose[6 * v + 3 + i];
        src.bind(v, cfg);
        const int nres = 2 * SRC::PER_ITEM * vinfo[4 * v];
        const bool fixa = cfg->fix_aspect != 0;
        const double aspect = cfg->aspect;
        double acc[5] = {0., 0., 0., 0., 0.}, e2 = 0.;
        for (int r0 = 0; r0 < nres; r0 += 64) {
            const int r = r0 + lane;
            if (r < nres) {
                double M[3];
                src.object(r, M);
                double *row = rows[lane];  // (cal_row stores the row's entries as it has them: no lane holds the 22 at once)
                // (the 36 doubles of the rotation are read where they are used: an offset the compiler cannot see through keeps it from
                // hoisting the loads out of the loop into 72 registers of every lane)
                int roff = 0;
                asm volatile("" : "+v"(roff));
                const double err = cal_row<MODEL>(M, rot + roff, rot + roff + 9, tv, K, kd, r & 1, row + 16, row) - src.image(r);
                row[22] = err;
                e2 += err * err;
                if (fixa) row[1] += aspect * row[0];
            }
            SR_LDS_SYNC();
            const int cnt = nres - r0 < 64 ? nres - r0 : 64;
            for (int i = 0; i < cnt; i++) {
#pragma unroll
                for (int q = 0; q < 5; q++) acc[q] += rows[i][ca[q]] * rows[i][cb[q]];
            }
            SR_LDS_SYNC();
        }
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const int e = lane + 64 * q;
            if (e < nent) {
                tri[e] = acc[q];
                blk[(size_t)v * CAL_TRI + e] = acc[q];
            }
        }
        e2 = wave_sum_f64(e2);
        if (lane == 0) cost[v] = e2;
    } else {
        for (int e = lane; e < nent; e += 64) tri[e] = blk[(size_t)v * CAL_TRI + e];
    }
    SR_LDS_SYNC();
    // ---- the Schur pieces under the current damping: lane j < nI has row j of W = B (C + lambda diag C)^-1
    const double lambda = final ? 0. : lm_lambda(st->lambdaLg10);
    double S[21], gP[6];
    {
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b = a; b < 6; b++) S[idx++] = tri[cal_tri(nI + a, nI + b, N)];
            gP[a] = tri[cal_tri(nI + a, nI + 6, N)];
        }
    }
    if (lane < nI) {
        double Bj[6], Wj[6];
#pragma unroll
        for (int a = 0; a < 6; a++) Bj[a] = tri[cal_tri(lane, nI + a, N)];
        solve6_spd(S, Bj, lambda, Wj);
        double rj = 0.;
#pragma unroll
        for (int a = 0; a < 6; a++) rj += Wj[a] * gP[a];
        sch[(size_t)v * CAL_SCH + 256 + lane] = rj;
        for (int k = 0; k < nI; k++) {
            double sjk = 0.;
#pragma unroll
            for (int a = 0; a < 6; a++) sjk += Wj[a] * tri[cal_tri(k, nI + a, N)];
            sch[(size_t)v * CAL_SCH + 16 * lane + k] = sjk;
        }
    }
}

// (launched with 64 threads; the never-launched upper bound makes the compiler aim for the occupancy four-wave workgroups would have
// under this LDS, i.e. schedule for few registers instead of settling at the 170 the one-wave workgroup's LDS would allow)
template <int MODEL>
__global__ WALKER_WG_ATTR(64, 1024) void k_calib_blocks(const CalCfg *__restrict__ cfg, const CalState *__restrict__ st, const fid_marker *__restrict__ markers,
                                                      const int2 *__restrict__ sel, const int *__restrict__ vinfo, const double *__restrict__ map_obj,
                                                      const double *__restrict__ pose, double *__restrict__ blk, double *__restrict__ sch,
                                                      double *__restrict__ cost, int final)
{
    cal_view_blocks<MODEL>(cfg, st, CalMarkers{markers, sel, map_obj, nullptr, nullptr}, vinfo, pose, blk, sch, cost, final);
}

// ------------------------------------------------------------------------------------------------ K23: the reduced system
// Threads 0 .. 255: entry (t / 16, t % 16) of A - sum W B^T; 256 .. 271: the right-hand side; 272: the cost.  Views in index order
// (the records of a view that is not used are zero and stay zero).  Then wave 0: Cholesky, a lane per row.
__global__ __launch_bounds__(320) void k_calib_solve(const CalCfg *__restrict__ cfg, CalState *__restrict__ st, const int *__restrict__ vinfo,
                                                      const double *__restrict__ blk, const double *__restrict__ sch, const double *__restrict__ cost,
                                                      const double *__restrict__ pose, int final, fid_calib_out *__restrict__ out,
                                                      fid_calib_view *__restrict__ vout)
{
    __shared__ double A[16][17], g[16], xs[16], Z[16][17], ctot;
    const int t = threadIdx.x;
    if (!final && st->done) return;
    const int nI = cfg->nI, N = nI + 7, nv = cfg->n_views;
    const double lambda = final ? 0. : lm_lambda(st->lambdaLg10);
    if (t < 256) {
        const int j = t >> 4, k = t & 15;
        if (j < nI && k <= j) {
            const int e = cal_tri(k, j, N);
            double sA = 0., sS = 0.;
#pragma unroll 8
            for (int v = 0; v < nv; v++) {
                sA += blk[(size_t)v * CAL_TRI + e];
                sS += sch[(size_t)v * CAL_SCH + t];
            }
            A[j][k] = (j == k ? sA * (1. + lambda) : sA) - sS;
        }
    } else if (t < 272) {
        const int j = t - 256;
        if (j < nI) {
            const int e = cal_tri(j, nI + 6, N);
            double sg = 0., sr = 0.;
#pragma unroll 8
            for (int v = 0; v < nv; v++) {
                sg += blk[(size_t)v * CAL_TRI + e];
                sr += sch[(size_t)v * CAL_SCH + 256 + j];
            }
            g[j] = sg - sr;
        }
    } else if (t == 272) {
        double s = 0.;
#pragma unroll 8
        for (int v = 0; v < nv; v++) s += cost[v];
        ctot = s;
    }
    __syncthreads();
    if (t >= 64) return;
    // ---- Cholesky of the lower triangle in place: lane t owns row t
    bool ok = true;
    for (int j = 0; j < nI; j++) {
        const double dj = A[j][j];
        if (!(dj > 0.) || !(dj - dj == 0.)) {  // (every lane reads the same value)
            ok = false;
            break;
        }
        const double sq = sqrt(dj);
        SR_LDS_SYNC();
        if (t == j) A[j][j] = sq;
        if (t > j && t < nI) A[t][j] = A[t][j] / sq;
        SR_LDS_SYNC();
        if (t > j && t < nI)
            for (int k = j + 1; k <= t; k++) A[t][k] -= A[t][j] * A[k][j];
        SR_LDS_SYNC();
    }
    if (!final) {
        if (t == 0) {
            double dn = 0., pn = 0.;
            if (ok) {
                for (int i = 0; i < nI; i++) {  // L y = g, L^T x = y
                    double s = g[i];
                    for (int k = 0; k < i; k++) s -= A[i][k] * xs[k];
                    xs[i] = s / A[i][i];
                }
                for (int i = nI - 1; i >= 0; i--) {
                    double s = xs[i];
                    for (int k = i + 1; k < nI; k++) s -= A[k][i] * xs[k];
                    xs[i] = s / A[i][i];
                }
                for (int i = 0; i < nI; i++) {
                    dn += xs[i] * xs[i];
                    pn += st->k[cfg->col[i]] * st->k[cfg->col[i]];
                }
            } else {
                for (int i = 0; i < nI; i++) xs[i] = 0.;
            }
            st->dnI = dn;
            st->pnI = pn;
            st->bad = ok ? 0 : 1;
            if (st->needJ) {
                st->cost = ctot;
                if (st->trials == 0) st->start_cost = ctot;
            }
        }
        SR_LDS_SYNC();
        if (t < nI) st->dI[t] = xs[t];
        if (t < 16) {  // the candidate's slot t
            double val = st->k[t];
            for (int j = 0; j < nI; j++)
                if (cfg->col[j] == t) val = st->k[t] - xs[j];
            if (t == 0 && cfg->fix_aspect)
                for (int j = 0; j < nI; j++)
                    if (cfg->col[j] == 1) val = cfg->aspect * (st->k[1] - xs[j]);
            st->cand[t] = val;
        }
        return;
    }
    // ---- FINAL: diag of the inverse = the squared column norms of L^-1; lane j solves L z = e_j in its row of Z
    const int n_free = nI + 6 * st->n_views_used, dof = 2 * st->n_points - n_free;
    const double s2 = dof > 0 ? ctot / (double)dof : 0.;
    double sd = 0.;
    if (ok && t < nI) {
        double nrm = 0.;
        for (int i = t; i < nI; i++) {
            double s = i == t ? 1. : 0.;
            for (int k = t; k < i; k++) s -= A[i][k] * Z[t][k];
            s /= A[i][i];
            Z[t][i] = s;
            nrm += s * s;
        }
        sd = sqrt(nrm * s2);
        if (!(sd - sd == 0.)) sd = 0.;
    }
    xs[t & 15] = 0.;
    SR_LDS_SYNC();
    if (t < nI) xs[t] = sd;
    SR_LDS_SYNC();
    if (t < 16) {
        double val = 0.;
        for (int j = 0; j < nI; j++)
            if (cfg->col[j] == t) val = xs[j];
        if (t == 0 && cfg->fix_aspect)
            for (int j = 0; j < nI; j++)
                if (cfg->col[j] == 1) val = fabs(cfg->aspect) * xs[j];
        out->std_dev[t] = val;
    }
    if (t == 0) {
        out->status = st->status;
        out->n_views_used = st->n_views_used;
        out->n_points = st->n_points;
        out->n_iter = st->trials;
        out->n_free = n_free;
        out->reserved0 = 0;
        out->cost = ctot;
        out->rms = st->n_points > 0 ? sqrt(ctot / (double)st->n_points) : 0.;
        out->start_cost = st->trials == 0 && st->needJ ? ctot : st->start_cost;
    }
    for (int v = t; v < nv; v += 64) {
        fid_calib_view o;
        o.status = vinfo[4 * v + 2];
        o.n_used = vinfo[4 * v];
        o.n_over = vinfo[4 * v + 1];
        o.reserved0 = 0;
        const bool used = o.status == FID_CALIB_VIEW_USED;
        for (int i = 0; i < 3; i++) {
            o.rvec[i] = used ? pose[6 * v + i] : 0.;
            o.tvec[i] = used ? pose[6 * v + 3 + i] : 0.;
        }
        o.rms = used ? sqrt(cost[v] / (double)(cfg->per_item * o.n_used)) : 0.;
        vout[v] = o;
    }
}

// ------------------------------------------------------------------------------------------------ K24: a view's candidate
// dnpn[2 v + ..]: |step|^2 and |pose|^2 of the view's six
template <int MODEL, class SRC>
__device__ __forceinline__ void cal_view_eval(const CalCfg *__restrict__ cfg, const CalState *__restrict__ st, SRC src, const int *__restrict__ vinfo,
                                              const double *__restrict__ pose, const double *__restrict__ blk, double *__restrict__ cand_pose,
                                              double *__restrict__ cand_cost, double *__restrict__ dnpn)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    if (st->done || st->bad) return;
    if (vinfo[4 * v + 2] != FID_CALIB_VIEW_USED) return;
    const int nI = cfg->nI, N = nI + 7;
    const double *tri = blk + (size_t)v * CAL_TRI;
    double S[21], rhs[6], param[6], dP[6];
    {
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b = a; b < 6; b++) S[idx++] = tri[cal_tri(nI + a, nI + b, N)];
            rhs[a] = tri[cal_tri(nI + a, nI + 6, N)];
        }
    }
    for (int j = 0; j < nI; j++) {
        const double dj = st->dI[j];
#pragma unroll
        for (int a = 0; a < 6; a++) rhs[a] -= tri[cal_tri(j, nI + a, N)] * dj;
    }
    solve6_spd(S, rhs, lm_lambda(st->lambdaLg10), dP);
    double dn = 0., pn = 0.;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double p0 = pose[6 * v + i];
        param[i] = p0 - dP[i];
        dn += dP[i] * dP[i];
        pn += p0 * p0;
    }
    const double K[9] = {st->cand[0], 0., st->cand[2], 0., st->cand[1], st->cand[3], 0., 0., 1.};
    double kd[12];
#pragma unroll
    for (int i = 0; i < 12; i++) kd[i] = st->cand[4 + i];
    src.bind(v, cfg);
    const int nres = 2 * SRC::PER_ITEM * vinfo[4 * v];
    double e2 = 0., R[9];
    cal_rotation_value(param, R);
    for (int r = lane; r < nres; r += 64) {
        double M[3];
        src.object(r, M);
        const double err = cal_project<MODEL>(M, R, param + 3, K, kd, r & 1) - src.image(r);
        e2 += err * err;
    }
    e2 = wave_sum_f64(e2);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) cand_pose[6 * v + i] = param[i];
        cand_cost[v] = e2;
        dnpn[2 * v] = dn;
        dnpn[2 * v + 1] = pn;
    }
}

template <int MODEL>
__global__ __launch_bounds__(64) void k_calib_eval(const CalCfg *__restrict__ cfg, const CalState *__restrict__ st, const fid_marker *__restrict__ markers,
                                                    const int2 *__restrict__ sel, const int *__restrict__ vinfo, const double *__restrict__ map_obj,
                                                    const double *__restrict__ pose, const double *__restrict__ blk, double *__restrict__ cand_pose,
                                                    double *__restrict__ cand_cost, double *__restrict__ dnpn)
{
    cal_view_eval<MODEL>(cfg, st, CalMarkers{markers, sel, map_obj, nullptr, nullptr}, vinfo, pose, blk, cand_pose, cand_cost, dnpn);
}

// ------------------------------------------------------------------------------------------------ K25: accept or reject, the stop
__global__ WALKER_WG_ATTR(64, 512) void k_calib_accept(const CalCfg *__restrict__ cfg, CalState *__restrict__ st, const int *__restrict__ vinfo,
                                                      double *__restrict__ pose, const double *__restrict__ cand_pose, const double *__restrict__ cand_cost,
                                                      const double *__restrict__ dnpn)
{
    __shared__ double sc[FID_CALIB_MAX_VIEWS], sd[FID_CALIB_MAX_VIEWS], sp[FID_CALIB_MAX_VIEWS];
    const int lane = threadIdx.x, nv = cfg->n_views;
    if (st->done) return;
    const bool bad = st->bad != 0;
    for (int v = lane; v < nv; v += 64) {
        const bool used = vinfo[4 * v + 2] == FID_CALIB_VIEW_USED && !bad;
        sc[v] = used ? cand_cost[v] : 0.;
        sd[v] = used ? dnpn[2 * v] : 0.;
        sp[v] = used ? dnpn[2 * v + 1] : 0.;
    }
    SR_LDS_SYNC();
    double cc = 0., dn = st->dnI, pn = st->pnI;  // the views in index order, the same in every lane
    for (int v = 0; v < nv; v++) {
        cc += sc[v];
        dn += sd[v];
        pn += sp[v];
    }
    int l = st->lambdaLg10, done = 0, status = FID_CALIB_OK;
    const int trials = st->trials + 1;
    const bool accept = !bad && cc - cc == 0. && !(cc > st->cost);
    if (accept) {
        for (int i = lane; i < 6 * nv; i += 64)
            if (vinfo[4 * (i / 6) + 2] == FID_CALIB_VIEW_USED) pose[i] = cand_pose[i];
        if (lane < 16) st->k[lane] = st->cand[lane];
        l = l - 1 > -16 ? l - 1 : -16;
        if (sqrt(dn) / (sqrt(pn) + DBL_EPSILON) < cfg->eps) done = 1;
    } else {
        l++;
        if (l > 16) {
            l = 16;
            done = 1;
            status = FID_CALIB_STALLED;
        }
    }
    if (!done && trials >= cfg->max_iter) {
        done = 1;
        status = FID_CALIB_MAX_ITER;
    }
    if (lane == 0) {
        if (accept) st->cost = cc;
        st->needJ = accept ? 1 : 0;
        st->lambdaLg10 = l;
        st->trials = trials;
        st->status = status;
        st->done = done;
    }
}

// ------------------------------------------------------------------------------------------------ host
struct CalibBufs {
    int cap_views = 0;
    DevArray<fid_marker> markers;
    DevBlock mem;  // everything below, sized by cap_views
    int *d_n = nullptr, *d_vinfo = nullptr;
    int2 *d_sel = nullptr;
    double *d_con = nullptr, *d_blk = nullptr, *d_sch = nullptr, *d_pose = nullptr, *d_cand = nullptr, *d_cost = nullptr, *d_ccost = nullptr, *d_dnpn = nullptr;
    fid_map_pose_out *d_vpose = nullptr;
    CalCfg *d_cfg = nullptr;
    CalState *d_state = nullptr;
    fid_calib_out *d_out = nullptr;
    fid_calib_view *d_vout = nullptr;
    size_t zero_from = 0, zero_bytes = 0;  // pose .. dnpn: zeroed at every call (a view that is not used adds nothing)
};

static void calib_free(fid_ctx *c)
{
    delete c->calib;
    c->calib = nullptr;
}

static fid_status calib_ensure(fid_ctx *c, int n_views, size_t n_markers)
{
    if (!c->calib) c->calib = new (std::nothrow) CalibBufs();
    CalibBufs *b = c->calib;
    if (!b) return FID_E_OUT_OF_MEMORY;
    HIPCHK(c, b->markers.reserve(n_markers));
    if (n_views > b->cap_views) {
        b->cap_views = 0;
        const size_t V = (size_t)n_views;
        MemLayout l;
        l.add(&b->d_cfg, 1), l.add(&b->d_state, 1), l.add(&b->d_out, 1), l.add(&b->d_n, V), l.add(&b->d_vinfo, 4 * V), l.add(&b->d_sel, MP_MAX_USED * V);
        l.add(&b->d_con, 6 * V), l.add(&b->d_vpose, V), l.add(&b->d_vout, V);
        b->zero_from = l.mark();
        l.add(&b->d_pose, 6 * V), l.add(&b->d_blk, CAL_TRI * V), l.add(&b->d_sch, CAL_SCH * V), l.add(&b->d_cand, 6 * V), l.add(&b->d_cost, V);
        l.add(&b->d_ccost, V), l.add(&b->d_dnpn, 2 * V);
        b->zero_bytes = l.mark() - b->zero_from;
        HIPCHK(c, b->mem.reserve(l.bytes()));
        l.bind(b->mem.p);
        b->cap_views = n_views;
    }
    return FID_OK;
}

void fid_default_calib_opts(fid_calib_opts *o)
{
    if (!o) return;
    o->free_mask = FID_CALIB_FREE_PLUMB_BOB;
    o->start = FID_CALIB_START_AUTO;
    o->fix_aspect = 0;
    o->min_markers = 1;
    o->max_iter = 100;
    o->reserved0 = 0;
    o->eps = 1e-12;
}

fid_status fid_camera_to_info(const fid_camera *cam, char *model_string, double K[9], double *D, int32_t *n_D)
{
    if (!fid_camera_usable(cam) || !model_string || !K || !D || !n_D) return FID_E_INVALID_ARG;
    const char *name = cam->model == FID_CAM_RATIONAL ? "rational_polynomial" : cam->model == FID_CAM_EQUIDISTANT ? "equidistant" : "plumb_bob";
    const int n = cam->model == FID_CAM_RATIONAL ? (cam->n_dist > 8 ? 12 : 8) : cam->model == FID_CAM_EQUIDISTANT ? 4 : 5;
    snprintf(model_string, 32, "%s", name);
    for (int i = 0; i < 9; i++) K[i] = cam->K[i];
    for (int i = 0; i < n; i++) D[i] = i < cam->n_dist ? cam->D[i] : 0.;
    *n_D = n;
    return FID_OK;
}

static bool calib_refuse(fid_ctx *c, const char *who, const std::string &why)
{
    c->last_error = std::string(who) + ": " + why;
    return true;
}

// ---- the steps fid_calibrate_map and fid_calibrate_charuco (fid_calib_points.hip) share; `who` names the entry point in the last error
// the arguments that do not depend on what a view holds -> whether the call is refused
static bool calib_refuse_args(fid_ctx *c, const char *who, const void *items, const int32_t *n_per_view, int32_t n_views, int32_t cap_per_view,
                              int32_t image_w, int32_t image_h, const fid_calib_opts *opts, const fid_camera *cam_io, const fid_calib_out *out)
{
    if (!items || !n_per_view || !opts || !cam_io || !out) return calib_refuse(c, who, "a NULL pointer");
    if (n_views < 1 || n_views > FID_CALIB_MAX_VIEWS)
        return calib_refuse(c, who, std::to_string(n_views) + " views: 1 .. " + std::to_string(FID_CALIB_MAX_VIEWS) + " (FID_CALIB_MAX_VIEWS)");
    if (cap_per_view < 1 || image_w < 1 || image_h < 1) return calib_refuse(c, who, "cap_per_view, image_w and image_h must be positive");
    if (!fid_camera_usable(cam_io)) return calib_refuse(c, who, "the camera's model or n_dist is outside the ABI's");
    if (opts->start != FID_CALIB_START_GIVEN && opts->start != FID_CALIB_START_AUTO) return calib_refuse(c, who, "start is neither GIVEN nor AUTO");
    if (!(opts->eps >= 0.) || opts->eps - opts->eps != 0. || opts->max_iter < 0 || opts->min_markers < 1)
        return calib_refuse(c, who, "eps must be finite and >= 0, max_iter >= 0, min_markers >= 1");
    const int n_slots = 4 + cam_io->n_dist;
    if (opts->free_mask >> n_slots)
        return calib_refuse(c, who, "free_mask names a slot beyond the camera's " + std::to_string(cam_io->n_dist) + " coefficients");
    return false;
}

// the start camera's values -> whether the call is refused
static bool calib_refuse_start(fid_ctx *c, const char *who, const fid_calib_opts *opts, const fid_camera &start)
{
    for (int i = 0; i < 9; i++)
        if (start.K[i] - start.K[i] != 0.) return calib_refuse(c, who, "the camera holds a value that is not finite");
    for (int i = 0; i < 12; i++)
        if (start.D[i] - start.D[i] != 0.) return calib_refuse(c, who, "the camera holds a value that is not finite");
    if (opts->fix_aspect != 0 && !(start.K[4] != 0.)) return calib_refuse(c, who, "fix_aspect needs fy != 0 in the camera");
    return false;
}

// the free slots and the rest of the device's configuration; *mask_out: the free slots as the solve takes them
static CalCfg calib_config(const fid_calib_opts *opts, const fid_camera &start, int n_views, int cap_per_view, int per_item, int min_items, unsigned *mask_out)
{
    const bool fixa = opts->fix_aspect != 0;
    CalCfg cfg = {};
    unsigned mask = opts->free_mask;
    if (fixa) mask &= ~1u;
    for (int i = 0; i < 16; i++)
        if (mask >> i & 1u) cfg.col[cfg.nI++] = i;
    cfg.fix_aspect = fixa && (mask >> 1 & 1u);
    cfg.aspect = fixa ? start.K[0] / start.K[4] : 1.;
    cfg.start_auto = opts->start == FID_CALIB_START_AUTO;
    cfg.min_markers = min_items;
    cfg.max_iter = opts->max_iter;
    cfg.n_views = n_views;
    cfg.per_view = cap_per_view;
    cfg.per_item = per_item;
    cfg.eps = opts->eps;
    *mask_out = mask;
    return cfg;
}

// START_AUTO's values into `start` from the views' flags and focal constraints (vinfo and con as the start kernel of the route left
// them): the rows of the views with at least cfg.min_markers used items and a homography (flag bit 1, and not bit 2: the point route's
// "on one line"), added in view order.  planar_or_refuse: a counted view without flag bit 0 refuses the call (the marker route).
static fid_status calib_auto_start(fid_ctx *c, const char *who, const CalCfg &cfg, unsigned mask, double cx0, double cy0, bool planar_or_refuse,
                                   fid_camera *start)
{
    CalibBufs *b = c->calib;
    hipStream_t st = c->stream;
    const int n_views = cfg.n_views;
    std::vector<int> vinfo((size_t)n_views * 4);
    std::vector<double> con((size_t)n_views * 6);
    HIPCHK(c, hipMemcpyAsync(vinfo.data(), b->d_vinfo, sizeof(int) * vinfo.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(con.data(), b->d_con, sizeof(double) * con.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    double aa = 0, ab = 0, bb = 0, ac = 0, bc = 0;
    for (int v = 0; v < n_views; v++) {
        if (vinfo[4 * (size_t)v] < cfg.min_markers) continue;
        const int flags = vinfo[4 * (size_t)v + 3];
        if (planar_or_refuse && !(flags & 1))
            return calib_refuse(c, who, "view " + std::to_string(v) + ": its mapped markers are not coplanar; START_AUTO needs planar views, give a start"),
                   FID_E_INVALID_ARG;
        if ((flags & 6) != 2) continue;
        for (int r = 0; r < 2; r++) {  // the view's two rows, in order
            const double *q = &con[6 * (size_t)v + 3 * r];
            aa += q[0] * q[0]; ab += q[0] * q[1]; bb += q[1] * q[1]; ac += q[0] * q[2]; bc += q[1] * q[2];
        }
    }
    const double det = aa * bb - ab * ab;
    const double X = (ac * bb - bc * ab) / det, Y = (aa * bc - ab * ac) / det;
    const double fx = sqrt(fabs(1. / X)), fy = sqrt(fabs(1. / Y));
    if (!(fx - fx == 0.) || !(fy - fy == 0.) || !(fx > 0.) || !(fy > 0.))
        return calib_refuse(c, who, "START_AUTO: the views do not determine the focal lengths; give a start"), FID_E_INVALID_ARG;
    if (mask >> 1 & 1u) start->K[4] = fy;
    if (mask & 1u) start->K[0] = fx;
    start->K[2] = cx0;
    start->K[5] = cy0;
    for (int i = 0; i < 12; i++)
        if (mask >> (4 + i) & 1u) start->D[i] = 0.;
    return FID_OK;
}

// From the start camera and the views' start-pose records to the caller's results: the state, the route's init kernel, the counts and
// their refusals, Levenberg-Marquardt in chunks of CAL_CHUNK trials, FINAL, the copies back.  init(), blocks(final) and eval() launch the
// route's K22 / K24 (and its form of k_calib_init) on the context's stream; k_calib_solve and k_calib_accept are launched here.
template <class INIT, class BLOCKS, class EVAL>
static fid_status calib_solve_views(fid_ctx *c, const char *who, const char *none_why, const CalCfg &cfg, unsigned mask, const fid_camera &start,
                                    INIT init, BLOCKS view_blocks, EVAL view_eval, fid_camera *cam_io, fid_calib_out *out, fid_calib_view *views)
{
    CalibBufs *b = c->calib;
    hipStream_t st = c->stream;
    const int n_views = cfg.n_views, max_iter = cfg.max_iter;
    CalState hs = {};
    hs.k[0] = start.K[0]; hs.k[1] = start.K[4]; hs.k[2] = start.K[2]; hs.k[3] = start.K[5];
    for (int i = 0; i < 12; i++) hs.k[4 + i] = start.D[i];
    for (int i = 0; i < 16; i++) hs.cand[i] = hs.k[i];
    hs.lambdaLg10 = -3;
    hs.needJ = 1;
    hs.done = max_iter == 0 ? 1 : 0;
    hs.status = max_iter == 0 ? FID_CALIB_MAX_ITER : FID_CALIB_OK;
    HIPCHK(c, hipMemcpyAsync(b->d_cfg, &cfg, sizeof(cfg), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(b->d_state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    init();
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&hs, b->d_state, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int n_free = cfg.nI + 6 * hs.n_views_used;
    if (hs.n_views_used == 0) return calib_refuse(c, who, none_why), FID_E_INVALID_ARG;
    if (2 * hs.n_points < n_free)
        return calib_refuse(c, who, std::to_string(2 * hs.n_points) + " residuals for " + std::to_string(n_free) + " free parameters"), FID_E_INVALID_ARG;
    // ---- Levenberg-Marquardt: CAL_CHUNK trials, then the status
    auto blocks = [&](int final) {
        view_blocks(final);
        hipLaunchKernelGGL(k_calib_solve, dim3(1), dim3(320), 0, st, (const CalCfg *)b->d_cfg, b->d_state, (const int *)b->d_vinfo, (const double *)b->d_blk,
                           (const double *)b->d_sch, (const double *)b->d_cost, (const double *)b->d_pose, final, b->d_out, b->d_vout);
    };
    int queued = 0;
    while (!hs.done) {
        for (int i = 0; i < CAL_CHUNK && queued < max_iter; i++, queued++) {
            blocks(0);
            view_eval();
            hipLaunchKernelGGL(k_calib_accept, dim3(1), dim3(64), 0, st, (const CalCfg *)b->d_cfg, b->d_state, (const int *)b->d_vinfo, b->d_pose,
                               (const double *)b->d_cand, (const double *)b->d_ccost, (const double *)b->d_dnpn);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&hs.lambdaLg10, &b->d_state->lambdaLg10, sizeof(int) * 4, hipMemcpyDeviceToHost, st));  // lambdaLg10 trials status done
        HIPCHK(c, hipStreamSynchronize(st));
        if (!hs.done && queued >= max_iter) {
            c->last_error = std::string(who) + ": the device did not report the stop after max_iter trials";
            return FID_E_HIP;
        }
    }
    blocks(1);
    HIPCHK(c, hipGetLastError());
    fid_calib_out ho;
    std::vector<fid_calib_view> hv((size_t)n_views);
    HIPCHK(c, hipMemcpyAsync(&ho, b->d_out, sizeof(ho), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&hs, b->d_state, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hv.data(), b->d_vout, sizeof(fid_calib_view) * (size_t)n_views, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // ---- the free slots into the caller's camera; every other byte of it stays
    unsigned written = mask;
    if (cfg.fix_aspect) written |= 1u;
    double *slot[16] = {&cam_io->K[0], &cam_io->K[4], &cam_io->K[2], &cam_io->K[5]};
    for (int i = 0; i < 12; i++) slot[4 + i] = &cam_io->D[i];
    for (int i = 0; i < 16; i++)
        if (written >> i & 1u) *slot[i] = hs.k[i];
    *out = ho;
    if (views) memcpy(views, hv.data(), sizeof(fid_calib_view) * (size_t)n_views);
    return FID_OK;
}

fid_status fid_calibrate_map(fid_ctx *c, const fid_marker *markers, const int32_t *n_per_view, int32_t n_views, int32_t cap_per_view, int32_t image_w,
                             int32_t image_h, const fid_calib_opts *opts, fid_camera *cam_io, fid_calib_out *out, fid_calib_view *views)
{
    static const char who[] = "fid_calibrate_map";
    if (!c) return FID_E_INVALID_ARG;
    if (calib_refuse_args(c, who, markers, n_per_view, n_views, cap_per_view, image_w, image_h, opts, cam_io, out)) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_map(c)) return FID_E_INVALID_ARG;
    fid_camera start = fid_camera_normalised(*cam_io);
    if (calib_refuse_start(c, who, opts, start)) return FID_E_INVALID_ARG;
    for (int v = 0; v < n_views; v++) {
        const int n = n_per_view[v] < 0 ? 0 : (n_per_view[v] > cap_per_view ? cap_per_view : n_per_view[v]);
        const fid_marker *m = markers + (size_t)v * cap_per_view;
        for (int i = 0; i < n; i++)
            for (int q = 0; q < 8; q++)
                if (m[i].corners[q] - m[i].corners[q] != 0.f)
                    return calib_refuse(c, who, "view " + std::to_string(v) + ", marker " + std::to_string(i) + ": a corner is not finite"), FID_E_INVALID_ARG;
    }
    unsigned mask = 0;
    const CalCfg cfg = calib_config(opts, start, n_views, cap_per_view, 4, opts->min_markers, &mask);

    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_markers = (size_t)n_views * cap_per_view;
    const fid_status rce = calib_ensure(c, n_views, n_markers);
    if (rce != FID_OK) return rce;
    CalibBufs *b = c->calib;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(b->markers.data(), markers, sizeof(fid_marker) * n_markers, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(b->d_n, n_per_view, sizeof(int) * (size_t)n_views, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(b->mem.p + b->zero_from, 0, b->zero_bytes, st));
    // ---- the views' used markers; with AUTO the focal constraints
    const double cx0 = (mask >> 2 & 1u) ? 0.5 * (image_w - 1) : start.K[2], cy0 = (mask >> 3 & 1u) ? 0.5 * (image_h - 1) : start.K[5];
    hipLaunchKernelGGL(k_calib_start, dim3(n_views), dim3(64), 0, st, (const fid_marker *)b->markers.data(), (const int *)b->d_n, cap_per_view,
                       (const int *)c->d_map_ids, (const double *)c->d_map_obj, c->map_n, cfg.start_auto, cx0, cy0, b->d_sel, b->d_vinfo, b->d_con);
    HIPCHK(c, hipGetLastError());
    if (cfg.start_auto) {
        const fid_status rca = calib_auto_start(c, who, cfg, mask, cx0, cy0, true, &start);
        if (rca != FID_OK) return rca;
    }
    if (cfg.fix_aspect) start.K[0] = cfg.aspect * start.K[4];
    // ---- the start poses: k_map_pose over the views under the start camera
    map_pose_launch(c, st, b->markers.data(), b->d_n, 1, cap_per_view, n_views, start, b->d_vpose);
    HIPCHK(c, hipGetLastError());
    const int model = start.model;
    return calib_solve_views(
        c, who, "no view can be used (too few mapped markers, or no start pose)", cfg, mask, start,
        [&] {
            hipLaunchKernelGGL(k_calib_init, dim3(1), dim3(64), 0, st, (const CalCfg *)b->d_cfg, b->d_state, b->d_vinfo, (const fid_map_pose_out *)b->d_vpose,
                               b->d_pose);
        },
        [&](int final) {
            POSE_CAM_DISPATCH(model, hipLaunchKernelGGL(k_calib_blocks<CAM_MODEL>, dim3(n_views), dim3(64), 0, st, (const CalCfg *)b->d_cfg,
                                                        (const CalState *)b->d_state, (const fid_marker *)b->markers.data(), (const int2 *)b->d_sel,
                                                        (const int *)b->d_vinfo, (const double *)c->d_map_obj, (const double *)b->d_pose, b->d_blk, b->d_sch,
                                                        b->d_cost, final));
        },
        [&] {
            POSE_CAM_DISPATCH(model, hipLaunchKernelGGL(k_calib_eval<CAM_MODEL>, dim3(n_views), dim3(64), 0, st, (const CalCfg *)b->d_cfg,
                                                        (const CalState *)b->d_state, (const fid_marker *)b->markers.data(), (const int2 *)b->d_sel,
                                                        (const int *)b->d_vinfo, (const double *)c->d_map_obj, (const double *)b->d_pose,
                                                        (const double *)b->d_blk, b->d_cand, b->d_ccost, b->d_dnpn));
        },
        cam_io, out, views);
}
