// fid_charuco.hip -- ChArUco boards (fid_abi.h: "ChArUco boards"): chessboard corners interpolated from the markers of a frame, refined by
// cornerSubPix, and the board pose over them.  Part of the fid_api.hip translation unit, behind fid_map_build.hip.  Nothing here is on
// the detect path: a context without a board allocates and launches nothing of it.
//
// ------------------------------------------------------------------------------------------------ k_charuco_interp: interpolation
// k_charuco_interp, one wave per frame (blockIdx.x: a batch is one launch):
//   (1) gather.  Lanes take the frame's marker list 64 at a time; the board's ids are first_id .. first_id + nm - 1, so the entry is
//       id - first_id.  As in k_map_pose a first pass marks every board marker that is hit (a bit per marker in LDS, a second hit sets
//       the marker's bit in a second table) and a second pass notes the list index of every marker hit exactly once.
//   (2) ROUTE = -1: lanes are markers -- the homography board plane -> image of every used marker (pnp_quad_homography on its four
//       corners, the marker's centre folded in), nine doubles per marker in LDS.  ROUTE = a camera model: the frame's board pose is
//       k_map_pose's record for the board's tables, computed by the launch in front of this one.
//   (3) lanes are chessboard corners, 64 at a time: position, window, selection; the kept ones are compacted in id order by ballot and
//       prefix count.
// k_charuco_subpix, one wave per (frame, kept corner): k_subpix's arithmetic with the item's own window (at most 10) -- the same tap
// order, the same five accumulators summed each by its own lane -- so the float corner is the sequential cornerSubPix bit for bit.
// k_charuco_pose, one wave per frame: its own exits (few corners, one line, a corner beyond the model) and point load, then fid_pnp.h's
// pnp_wave_solve -- the solve of k_map_pose -- over ChPoseView, single points with z = 0: a planar-only view, so the planarity test and
// the start of a set that is not coplanar are not compiled.
#include <algorithm>

#define CH_MAX_MARKERS FID_MAP_MAX_USED
#define CH_MAX_CORNERS FID_CHARUCO_MAX_SQUARES  // (squares_x - 1) (squares_y - 1) < squares_x squares_y
#define CH_MAXWIN 10
#define CH_MASK_STRIDE ((2 * CH_MAXWIN + 1) * (2 * CH_MAXWIN + 1))
#define CH_SUBPIX_ITERS 30
#define CH_SUBPIX_EPS 0.1

// the board on the device: per chessboard corner {nearest marker a, nearest marker b, corner of a, corner of b}, the markers' object
// points as k_map_pose takes a map's (12 doubles a marker), the chessboard corners' (3 doubles)
struct ChBoardDev {
    const int *near4;
    const double *mobj;
    const double *cobj;
    int nm, nc, first_id;
};

struct ChInterpLds {
    double Hm[CH_MAX_MARKERS][9];
    int midx[CH_MAX_MARKERS];
    unsigned seen[CH_MAX_MARKERS / 32], dup[CH_MAX_MARKERS / 32];
};

template <int ROUTE>
__global__ __launch_bounds__(64) void k_charuco_interp(const fid_marker *__restrict__ markers, const int *__restrict__ nmark_per_frame, int nmark_stride_ints,
                                                        int per_frame, ChBoardDev b, PoseCam cam, const fid_map_pose_out *__restrict__ bpose, int W, int H,
                                                        int min_markers, fid_charuco_corner *__restrict__ out, int out_stride, int *__restrict__ n_out)
{
    __shared__ ChInterpLds s;
    const int f = blockIdx.x, lane = threadIdx.x;
    const fid_marker *mlist = markers + (long long)f * per_frame;
    int nm = nmark_per_frame[(long long)f * nmark_stride_ints];
    nm = nm < 0 ? 0 : (nm > per_frame ? per_frame : nm);
    const int bm = b.nm > CH_MAX_MARKERS ? CH_MAX_MARKERS : b.nm, bc = b.nc > CH_MAX_CORNERS ? CH_MAX_CORNERS : b.nc;
    // ---- (1) the frame's markers that the board names, without the ids seen twice
    for (int e = lane; e < CH_MAX_MARKERS / 32; e += 64) s.seen[e] = s.dup[e] = 0u;
    for (int k = lane; k < CH_MAX_MARKERS; k += 64) s.midx[k] = -1;
    SR_LDS_SYNC();
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        const long long k = m < nm ? (long long)mlist[m].id - b.first_id : -1;
        if (k >= 0 && k < bm) {
            const unsigned bit = 1u << (k & 31);
            if (atomicOr(&s.seen[k >> 5], bit) & bit) atomicOr(&s.dup[k >> 5], bit);
        }
    }
    SR_LDS_SYNC();
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        const long long k = m < nm ? (long long)mlist[m].id - b.first_id : -1;
        if (k >= 0 && k < bm && !(s.dup[k >> 5] >> (k & 31) & 1u)) s.midx[k] = m;
    }
    SR_LDS_SYNC();
    double param[6] = {0, 0, 0, 0, 0, 0};
    if constexpr (ROUTE < 0) {
        // ---- (2) lanes are markers: board plane -> image through the marker's four corners
        for (int k = lane; k < bm; k += 64) {
            const int m = s.midx[k];
            if (m < 0) continue;
            const double *o = b.mobj + (size_t)k * 12;
            const float *ic = mlist[m].corners;
            const double ix[4] = {(double)ic[0], (double)ic[2], (double)ic[4], (double)ic[6]};
            const double iy[4] = {(double)ic[1], (double)ic[3], (double)ic[5], (double)ic[7]};
            const double wx = o[3] - o[0], wy = o[1] - o[10];  // corner 0 -> 1 along x, corner 3 -> 0 along y
            const double ccx = 0.5 * (o[0] + o[6]), ccy = 0.5 * (o[1] + o[7]);
            double h[9];
            bool ok = pnp_quad_homography(ix, iy, 1. / wx, 1. / wy, h);
            for (int i = 0; i < 9; i++) ok = ok && h[i] - h[i] == 0.;
            if (!ok) {
                s.midx[k] = -1;  // (no homography: the marker counts as not detected)
                continue;
            }
            // h takes (X - ccx, Y - ccy): fold the centre in
            for (int r = 0; r < 3; r++) h[3 * r + 2] = h[3 * r + 2] - h[3 * r] * ccx - h[3 * r + 1] * ccy;
            for (int i = 0; i < 9; i++) s.Hm[k][i] = h[i];
        }
        SR_LDS_SYNC();
    } else {
        const fid_map_pose_out bp = bpose[f];
        bool ok = bp.n_markers > 0 && !(bp.image_error < 0.);
        for (int i = 0; i < 3; i++) {
            param[i] = bp.rvec[i];
            param[3 + i] = bp.tvec[i];
            ok = ok && bp.rvec[i] - bp.rvec[i] == 0. && bp.tvec[i] - bp.tvec[i] == 0.;
        }
        if (!ok) {  // (wave-uniform) no board pose, or the void fisheye record: no corners
            if (lane == 0) n_out[f] = 0;
            return;
        }
    }
    // ---- (3) lanes are chessboard corners
    int kept = 0;
    fid_charuco_corner *dst = out + (long long)f * out_stride;
    for (int i0 = 0; i0 < bc; i0 += 64) {
        const int i = i0 + lane;
        bool keep = false;
        float x0 = 0.f, y0 = 0.f;
        int win = 1;
        if (i < bc) {
            const int4 nr = *reinterpret_cast<const int4 *>(b.near4 + 4 * (size_t)i);
            const int mk[2] = {nr.x, nr.y}, cn[2] = {nr.z, nr.w};
            const double X = b.cobj[3 * (size_t)i], Y = b.cobj[3 * (size_t)i + 1];
            int ndet = 0;
            float px[2], py[2];
            for (int a = 0; a < 2; a++) {
                const int k = mk[a];
                if (k < 0 || k >= bm || s.midx[k] < 0) continue;
                if constexpr (ROUTE < 0) {
                    const double *h = s.Hm[k];
                    const double w = h[6] * X + h[7] * Y + h[8];
                    px[ndet] = (float)((h[0] * X + h[1] * Y + h[2]) / w);
                    py[ndet] = (float)((h[3] * X + h[4] * Y + h[5]) / w);
                }
                ndet++;
            }
            if constexpr (ROUTE < 0) {
                if (ndet == 2) {
                    x0 = (px[0] + px[1]) / 2.f;
                    y0 = (py[0] + py[1]) / 2.f;
                } else if (ndet == 1) {
                    x0 = px[0];
                    y0 = py[0];
                }
            } else {
                const double M[3] = {X, Y, b.cobj[3 * (size_t)i + 2]};
                double Jrow[6];
                x0 = (float)project_one<(ROUTE < 0 ? 0 : ROUTE)>(M, param, cam.K, cam.D, 0, Jrow, false);
                y0 = (float)project_one<(ROUTE < 0 ? 0 : ROUTE)>(M, param, cam.K, cam.D, 1, Jrow, false);
            }
            // the window: the nearest image corner of the detected nearest markers
            double minDist = -1.;
            for (int a = 0; a < 2; a++) {
                const int k = mk[a];
                if (k < 0 || k >= bm || s.midx[k] < 0) continue;
                const float *ic = mlist[s.midx[k]].corners;
                const float dx = x0 - ic[2 * cn[a]], dy = y0 - ic[2 * cn[a] + 1];
                const double dist = sqrt((double)dx * dx + (double)dy * dy);
                if (minDist == -1. || dist < minDist) minDist = dist;
            }
            const double wd = minDist - 2.;
            win = !(wd >= 1.) ? 1 : (wd >= (double)CH_MAXWIN ? CH_MAXWIN : (int)wd);
            keep = ndet >= 1 && ndet >= min_markers && x0 >= 2.f && x0 < (float)(W - 2) && y0 >= 2.f && y0 < (float)(H - 2);
        }
        const unsigned long long hit = __ballot(keep);
        if (keep) {
            const int pos = kept + __builtin_popcountll(hit & ((1ull << lane) - 1ull));
            if (pos < out_stride) {
                fid_charuco_corner r;
                r.id = i;
                r.win = win;
                r.x = r.x0 = x0;
                r.y = r.y0 = y0;
                dst[pos] = r;
            }
        }
        kept += __builtin_popcountll(hit);
    }
    if (lane == 0) n_out[f] = kept > out_stride ? out_stride : kept;
}

// ------------------------------------------------------------------------------------------------ k_charuco_subpix: refinement
// cornerSubPix (cornersubpix.cpp) with getRectSubPix 8u -> 32f (samplers.cpp), k_subpix restated for a window that comes with the item:
// blockIdx.x = the slot among the frame's kept corners, blockIdx.y = the frame.  maskw: the weight masks of the windows 1 .. CH_MAXWIN,
// CH_MASK_STRIDE floats each, made on the host as cornersubpix.cpp makes them.
__global__ __launch_bounds__(64) void k_charuco_subpix(const uint8_t *__restrict__ gray, long long gfstride, int gs, int W, int H,
                                                        fid_charuco_corner *__restrict__ corners, int out_stride, const int *__restrict__ n_out,
                                                        const float *__restrict__ maskw)
{
    constexpr int SP_NK = (CH_MASK_STRIDE + 63) / 64;
    __shared__ float sp[(2 * CH_MAXWIN + 3) * (2 * CH_MAXWIN + 3)];
    constexpr int SP_NTP = (CH_MASK_STRIDE + 15) & ~15;
    __shared__ __attribute__((aligned(16))) double prod[5][SP_NTP];
    constexpr int SP_CMAX = (2 * CH_MAXWIN + 3) + 1 + 2 * (CH_MAXWIN + 1);
    __shared__ uint8_t s_img[SP_CMAX * SP_CMAX];
    __shared__ float s_c[2];
    __shared__ int s_flag;
    const int lane = threadIdx.x, f = blockIdx.y, item = blockIdx.x;
    if (item >= n_out[f] || item >= out_stride) return;
    fid_charuco_corner *rec = corners + (long long)f * out_stride + item;
    int win = rec->win;
    win = win < 1 ? 1 : (win > CH_MAXWIN ? CH_MAXWIN : win);
    const int ww = 2 * win + 1, pw = ww + 2;
    const float *mw = maskw + (size_t)(win - 1) * CH_MASK_STRIDE;
    const uint8_t *g = gray + (long long)f * gfstride;
    // (rows padded to a multiple of 16 taps; the pad holds -0.0, the one value x + pad == x holds for bit for bit, for every x)
    for (int t = ww * ww + lane; t < SP_NTP; t += 64)
#pragma unroll
        for (int q = 0; q < 5; q++) prod[q][t] = -0.0;
    const float cTx = rec->x0, cTy = rec->y0;
    float cIx = cTx, cIy = cTy;
    // the gray pixels every iteration's patch can touch while the corner stays within win + 1 pixels of where it started, fetched once
    const int cm = win + 1, csz = pw + 1 + 2 * cm;
    const int X0 = (int)floorf(cTx - (pw - 1) * 0.5f) - cm, Y0 = (int)floorf(cTy - (pw - 1) * 0.5f) - cm;
    const bool cached = X0 >= 0 && Y0 >= 0 && X0 + csz <= W && Y0 + csz <= H;
    if (cached)
        for (int p = lane; p < csz * csz; p += 64) {
            const int i = p / csz, j = p - i * csz;
            s_img[p] = g[(long long)(Y0 + i) * gs + X0 + j];
        }
    float wgt[SP_NK];
#pragma unroll
    for (int k = 0; k < SP_NK; k++) wgt[k] = lane + 64 * k < ww * ww ? mw[lane + 64 * k] : 0.f;
    int iter = 0;
    for (;;) {
        // getRectSubPix(src, (pw, pw), cI) -> sp
        const float cx = cIx - (pw - 1) * 0.5f, cy = cIy - (pw - 1) * 0.5f;
        const int ipx = (int)floorf(cx), ipy = (int)floorf(cy);
        __syncthreads();
        if (cached && ipx >= X0 && ipy >= Y0 && ipx + pw + 1 <= X0 + csz && ipy + pw + 1 <= Y0 + csz) {
            // the fast path below, pixels from the LDS copy (same arithmetic)
            float a = cx - ipx, b = cy - ipy;
            a = a > 0.0001f ? a : 0.0001f;
            const float a12 = a * (1.f - b), a22 = a * b, b1 = 1.f - b, b2 = b;
            const double sc = (1. - a) / a;
            const uint8_t *s0 = s_img + (ipy - Y0) * csz + (ipx - X0);
            for (int p = lane; p < pw * pw; p += 64) {
                const int i = p / pw, j = p - i * pw;
                const uint8_t *q = s0 + i * csz + j;
                const float t = a12 * q[1] + a22 * q[1 + csz];
                float prev;
                if (j == 0) {
                    prev = (1 - a) * (b1 * q[0] + b2 * q[csz]);
                } else {
                    const float tp = a12 * q[0] + a22 * q[csz];
                    prev = (float)(tp * sc);
                }
                sp[p] = prev + t;
            }
        } else if (0 <= ipx && ipx + pw < W && 0 <= ipy && ipy + pw < H) {
            // getRectSubPix_8u32f fast path: dst[j] = prev_j + t_j, prev_0 = (1-a)(b1 s[0] + b2 s[step]),
            // prev_j = (float)(t_{j-1} * s), t_j = a12 s[j+1] + a22 s[j+1+step]
            float a = cx - ipx, b = cy - ipy;
            a = a > 0.0001f ? a : 0.0001f;
            const float a12 = a * (1.f - b), a22 = a * b, b1 = 1.f - b, b2 = b;
            const double sc = (1. - a) / a;
            const uint8_t *s0 = g + (long long)ipy * gs + ipx;
            for (int p = lane; p < pw * pw; p += 64) {
                const int i = p / pw, j = p - i * pw;
                const uint8_t *sr = s0 + (long long)i * gs;
                const float t = a12 * sr[j + 1] + a22 * sr[j + 1 + gs];
                float prev;
                if (j == 0) {
                    prev = (1 - a) * (b1 * sr[0] + b2 * sr[gs]);
                } else {
                    const float tp = a12 * sr[j] + a22 * sr[j + gs];
                    prev = (float)(tp * sc);
                }
                sp[p] = prev + t;
            }
        } else {
            // getRectSubPix_Cn_ with replicated border (adjustRect semantics == clamped coordinates)
            const float a = cx - ipx, b = cy - ipy;
            const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b;
            const float b1 = 1.f - b, b2 = b;
            const int inside = 0 <= ipx && ipx < W - pw && 0 <= ipy && ipy < H - pw;
            // emulate adjustRect: r = [rx, rw) x [ry, rh) are the columns/rows that interpolate normally
            int rx, ry, rw, rh;
            long long basey = 0, basex = 0;
            {
                const int x = ipx, y = ipy;
                if (y >= 0) { basey += y; ry = 0; } else ry = -y < pw ? -y : pw;
                if (y + pw < H) rh = pw; else { rh = H - y - 1; if (rh < 0) { basey += rh; rh = 0; } }
                if (x >= 0) { basex += x; rx = 0; } else rx = -x < pw ? -x : pw;
                if (x + pw < W) rw = pw; else { rw = W - x - 1; if (rw < 0) { basex += rw; rw = 0; } }
                basex -= rx;
            }
            for (int p = lane; p < pw * pw; p += 64) {
                const int i = p / pw, j = p - i * pw;
                float v;
                if (inside) {
                    const uint8_t *sr = g + (long long)(ipy + i) * gs + ipx;
                    v = sr[j] * a11 + sr[j + 1] * a12 + sr[j + gs] * a21 + sr[j + gs + 1] * a22;
                } else {
                    // row pointer after i iterations of the reference loop: src advances only while ry <= row < rh
                    const int lo = ry, hi = rh < i ? rh : i;
                    const int adv = hi > lo ? hi - lo : 0;
                    const long long y0r = basey + adv;
                    const long long y1r = (i < ry || i >= rh) ? y0r : y0r + 1;
                    const uint8_t *sr = g + y0r * gs + basex;
                    const uint8_t *sr2 = g + y1r * gs + basex;
                    if (j < rx) v = sr[rx] * b1 + sr2[rx] * b2;
                    else if (j < rw) v = sr[j] * a11 + sr[j + 1] * a12 + sr2[j] * a21 + sr2[j + 1] * a22;
                    else v = sr[rw] * b1 + sr2[rw] * b2;
                }
                sp[p] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SP_NK; k++) {
            const int t = lane + 64 * k;
            if (t >= ww * ww) break;
            const int i = t / ww, j = t - i * ww;
            const float *q = sp + (i + 1) * pw + (j + 1);
            const double m = wgt[k];
            const double tgx = q[1] - q[-1];
            const double tgy = q[pw] - q[-pw];
            const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
            const double px = j - win, py = i - win;
            prod[0][t] = gxx;
            prod[1][t] = gxy;
            prod[2][t] = gyy;
            prod[3][t] = gxx * px + gxy * py;
            prod[4][t] = gxy * px + gyy * py;
        }
        __syncthreads();
        // the five accumulators are summed in the reference's tap order, one accumulator per lane (0..4); whole groups of sixteen: the
        // row's pad is -0.0
        double accv = 0;
        if (lane < 5) {
            const double *pr = prod[lane];
            const int nt = ww * ww;
            for (int t0 = 0; t0 < nt; t0 += 16) {
                double v[16];
#pragma unroll
                for (int k = 0; k < 16; k++) v[k] = pr[t0 + k];
#pragma unroll
                for (int k = 0; k < 16; k++) accv += v[k];
            }
        }
        const double a = bcast_f64(accv, 0), b = bcast_f64(accv, 1), c = bcast_f64(accv, 2);
        const double bb1 = bcast_f64(accv, 3), bb2 = bcast_f64(accv, 4);
        if (lane == 0) {
            int flag = 0;  // 1 stop, 2 moved
            const double det = a * c - b * b;
            if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) {
                flag = 1;
            } else {
                const double scale = 1.0 / det;
                const float nx = (float)(cIx + c * scale * bb1 - b * scale * bb2);
                const float ny = (float)(cIy - b * scale * bb1 + a * scale * bb2);
                const double err = (nx - cIx) * (nx - cIx) + (ny - cIy) * (ny - cIy);
                s_c[0] = nx;
                s_c[1] = ny;
                if (nx < 0 || nx >= W || ny < 0 || ny >= H) flag = 1;
                else if (!(iter + 1 < CH_SUBPIX_ITERS && err > CH_SUBPIX_EPS * CH_SUBPIX_EPS)) flag = 1;
                flag |= 2;
            }
            s_flag = flag;
        }
        __syncthreads();
        const int flag = s_flag;
        if (flag & 2) {
            cIx = s_c[0];
            cIy = s_c[1];
        }
        iter++;
        if (flag & 1) break;
    }
    if (fabsf(cIx - cTx) > win || fabsf(cIy - cTy) > win) {
        cIx = cTx;
        cIy = cTy;
    }
    if (lane == 0) {
        rec->x = cIx;
        rec->y = cIy;
    }
}

// ------------------------------------------------------------------------------------------------ k_charuco_pose: the board pose over the corners
struct ChPoseLds {
    double obj[CH_MAX_CORNERS][2], img[CH_MAX_CORNERS][2];
    float mn[CH_MAX_CORNERS][2], Mxy[CH_MAX_CORNERS][2];
    double A[81], V[81];
};

// fid_pnp.h's view of the corners: the tables as they stand, z = 0 on the board (a planar-only view: no markers, no areas)
struct ChPoseView {
    ChPoseLds *s;
    static constexpr bool PLANAR_ONLY = true;
    __device__ __forceinline__ void obj(int i, double M[3]) const
    {
        M[0] = s->obj[i][0];
        M[1] = s->obj[i][1];
        M[2] = 0.;
    }
    __device__ __forceinline__ double img(int i, int c) const { return s->img[i][c]; }
    __device__ __forceinline__ float mn(int i, int c) const { return s->mn[i][c]; }
    __device__ __forceinline__ float *Mxy(int i) const { return s->Mxy[i]; }
    __device__ __forceinline__ double *A() const { return s->A; }
    __device__ __forceinline__ double *V() const { return s->V; }
};

__device__ __forceinline__ void ch_pose_none(fid_charuco_pose_out *o, int n, int status)
{
    fid_charuco_pose_out r;
    r.n_corners = n;
    r.status = status;
    pnp_pose_record_zero(r, 0.);
    *o = r;
}

template <int MODEL>
__global__ __launch_bounds__(64) void k_charuco_pose(const fid_charuco_corner *__restrict__ corners, int out_stride, const int *__restrict__ n_per_frame,
                                                      const double *__restrict__ cobj, int nc, int row_len, PoseCam cam,
                                                      fid_charuco_pose_out *__restrict__ out)
{
    __shared__ ChPoseLds s;
    const int f = blockIdx.x, lane = threadIdx.x;
    const double *K = cam.K, *kd = cam.D;
    const fid_charuco_corner *src = corners + (long long)f * out_stride;
    int n = n_per_frame[f];
    n = n < 0 ? 0 : (n > out_stride ? out_stride : (n > CH_MAX_CORNERS ? CH_MAX_CORNERS : n));
    if (n < 4) {
        if (lane == 0) ch_pose_none(out + f, n, FID_CHARUCO_POSE_FEW);
        return;
    }
    // ---- all corners on one line of the grid?  exactly, on the integer (cx, cy): the first corner that is not the first one gives the
    // direction, every corner's cross product with it must vanish
    {
        int id0 = src[0].id;
        id0 = id0 < 0 ? 0 : (id0 >= nc ? nc - 1 : id0);
        const int x0 = id0 % row_len, y0 = id0 / row_len;
        int first = n;
        for (int p = lane; p < n; p += 64) {
            int id = src[p].id;
            id = id < 0 ? 0 : (id >= nc ? nc - 1 : id);
            if ((id % row_len != x0 || id / row_len != y0) && p < first) first = p;
        }
        for (int mask = 1; mask < 64; mask <<= 1) {
            const int o = __shfl_xor(first, mask, WAVE);
            first = o < first ? o : first;
        }
        bool off_line = false;
        if (first < n) {
            int id1 = src[first].id;
            id1 = id1 < 0 ? 0 : (id1 >= nc ? nc - 1 : id1);
            const int dx = id1 % row_len - x0, dy = id1 / row_len - y0;
            for (int p = lane; p < n; p += 64) {
                int id = src[p].id;
                id = id < 0 ? 0 : (id >= nc ? nc - 1 : id);
                off_line = off_line || dx * (id / row_len - y0) - dy * (id % row_len - x0) != 0;
            }
        }
        if (__ballot(off_line) == 0ull) {
            if (lane == 0) ch_pose_none(out + f, n, FID_CHARUCO_POSE_COLLINEAR);
            return;
        }
    }
    // ---- the points: object (x, y; z = 0 on the board), image, the undistorted image point rounded to float (findHomography's input)
    bool posable = true;
    for (int p = lane; p < n; p += 64) {
        int id = src[p].id;
        id = id < 0 ? 0 : (id >= nc ? nc - 1 : id);
        s.obj[p][0] = cobj[3 * (size_t)id];
        s.obj[p][1] = cobj[3 * (size_t)id + 1];
        const double u = (double)src[p].x, v = (double)src[p].y;
        s.img[p][0] = u;
        s.img[p][1] = v;
        double x, y;
        const bool ok = pnp_undistort<MODEL>(K, kd, u, v, &x, &y);
        if constexpr (MODEL == FID_CAM_EQUIDISTANT) posable = posable && ok;
        s.mn[p][0] = (float)x;
        s.mn[p][1] = (float)y;
    }
    SR_LDS_SYNC();
    if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
        if (__ballot(!posable) != 0ull) {
            if (lane == 0) ch_pose_none(out + f, n, FID_CHARUCO_POSE_VOID);
            return;
        }
    }
    // ---- the plane's frame, the DLT start, CvLevMarq and the reprojection error over the corners
    double param[6], image_error;
    pnp_wave_solve<MODEL>(ChPoseView{&s}, n, lane, K, kd, param, &image_error);
    if (lane == 0) {
        fid_charuco_pose_out o;
        o.n_corners = n;
        o.status = FID_CHARUCO_POSE_OK;
        pnp_pose_record(o, param, image_error);
        out[f] = o;
    }
}

// ------------------------------------------------------------------------------------------------ host
// everything the board needs on a context (nothing of it exists until the first board is set): the board's tables, the window masks,
// max_batch + 1 frames of results (the slot behind a batch's serves the calls that bring their input from the host), staging
struct CharucoBufs {
    fid_charuco_board board = {};
    int nm = 0, nc = 0;  // nm == 0: no board
    int *d_ids = nullptr, *d_near = nullptr, *d_n = nullptr;
    double *d_mobj = nullptr, *d_cobj = nullptr;
    float *d_mask = nullptr;
    fid_charuco_corner *d_corners = nullptr;
    fid_map_pose_out *d_bposes = nullptr;
    fid_charuco_pose_out *d_cposes = nullptr;
    DevBlock mem;  // everything above
    DevArray<uint8_t> img;
    MarkerStage in;
    std::vector<fid_charuco_corner> h_corners;
    std::vector<int> h_n;
};

static void charuco_free(fid_ctx *c)
{
    delete c->charuco;
    c->charuco = nullptr;
}

// cornerSubPix's weight masks for the windows 1 .. CH_MAXWIN, as cornersubpix.cpp makes them (float expf): k_charuco_subpix's table
static std::vector<float> charuco_subpix_masks()
{
    std::vector<float> mask((size_t)CH_MASK_STRIDE * CH_MAXWIN, 0.f);
    for (int win = 1; win <= CH_MAXWIN; win++) {
        const int ww = 2 * win + 1;
        float *m = mask.data() + (size_t)(win - 1) * CH_MASK_STRIDE;
        for (int i = 0; i < ww; i++) {
            const float y = (float)(i - win) / win;
            const float vy = expf(-y * y);
            for (int j = 0; j < ww; j++) {
                const float x = (float)(j - win) / win;
                m[(size_t)i * ww + j] = (float)(vy * expf(-x * x));
            }
        }
    }
    return mask;
}

static bool refuse_no_board(fid_ctx *c)
{
    const bool none = !c->charuco || c->charuco->nm == 0;
    if (none) c->last_error = "no ChArUco board: fid_set_charuco_board first";
    return none;
}

fid_status fid_set_charuco_board(fid_ctx *c, const fid_charuco_board *board)
{
    if (!c || refuse_in_flight(c)) return FID_E_INVALID_ARG;
    if (!board) {
        if (c->charuco) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->charuco->nm = c->charuco->nc = 0;
        }
        return FID_OK;
    }
    const int sx = board->squares_x, sy = board->squares_y;
    const double sl = board->square_len, ml = board->marker_len;
    if (sx < 2 || sy < 2) {
        c->last_error = "ChArUco board of " + std::to_string(sx) + " x " + std::to_string(sy) + " squares: at least 2 a side";
        return FID_E_INVALID_ARG;
    }
    if ((long long)sx * sy > FID_CHARUCO_MAX_SQUARES) {
        c->last_error = "ChArUco board of " + std::to_string(sx) + " x " + std::to_string(sy) + " squares: at most " +
                        std::to_string(FID_CHARUCO_MAX_SQUARES) + " squares (FID_CHARUCO_MAX_SQUARES: " + std::to_string(FID_MAP_MAX_USED) +
                        " markers enter one board pose)";
        return FID_E_UNSUPPORTED;
    }
    if (!(sl - sl == 0) || !(ml - ml == 0) || !(ml > 0) || !(ml < sl)) {
        c->last_error = "ChArUco board: marker_len must lie inside (0, square_len) and both be finite";
        return FID_E_INVALID_ARG;
    }
    const int nm = sx * sy / 2, nc = (sx - 1) * (sy - 1);
    if (board->first_id < 0 || (long long)board->first_id + nm > c->dict_n) {
        c->last_error = "ChArUco board: ids " + std::to_string(board->first_id) + " .. " + std::to_string((long long)board->first_id + nm - 1) +
                        " are not all inside the context's dictionary of " + std::to_string(c->dict_n) + " markers";
        return FID_E_INVALID_ARG;
    }
    // the tables, as fid_abi.h states them
    std::vector<int> ids((size_t)nm), near4((size_t)nc * 4), marker_at((size_t)sx * sy, -1);
    std::vector<double> mobj((size_t)nm * 12), cobj((size_t)nc * 3);
    const double d = (sl - ml) / 2;
    int k = 0;
    for (int y = 0; y < sy; y++)
        for (int x = 0; x < sx; x++) {
            if ((x + y) % 2 == 0) continue;
            marker_at[(size_t)y * sx + x] = k;
            ids[(size_t)k] = board->first_id + k;
            const double c0x = x * sl + d, c0y = y * sl + d + ml;
            const double px[4] = {c0x, c0x + ml, c0x + ml, c0x}, py[4] = {c0y, c0y, c0y - ml, c0y - ml};
            for (int q = 0; q < 4; q++) {
                mobj[(size_t)k * 12 + q * 3] = (double)(float)px[q];
                mobj[(size_t)k * 12 + q * 3 + 1] = (double)(float)py[q];
                mobj[(size_t)k * 12 + q * 3 + 2] = 0.;
            }
            k++;
        }
    for (int cy = 0; cy < sy - 1; cy++)
        for (int cx = 0; cx < sx - 1; cx++) {
            const int i = cy * (sx - 1) + cx;
            const double X = (double)(float)((cx + 1) * sl), Y = (double)(float)((cy + 1) * sl);
            cobj[(size_t)i * 3] = X;
            cobj[(size_t)i * 3 + 1] = Y;
            cobj[(size_t)i * 3 + 2] = 0.;
            int a, b;
            if ((cx + cy) % 2 == 0) {
                a = marker_at[(size_t)cy * sx + cx + 1];
                b = marker_at[(size_t)(cy + 1) * sx + cx];
            } else {
                a = marker_at[(size_t)cy * sx + cx];
                b = marker_at[(size_t)(cy + 1) * sx + cx + 1];
            }
            if (a > b) std::swap(a, b);
            const int mk[2] = {a, b};
            for (int w = 0; w < 2; w++) {
                int best = 0;
                double bd = -1.;
                for (int q = 0; q < 4; q++) {
                    const double dx = mobj[(size_t)mk[w] * 12 + q * 3] - X, dy = mobj[(size_t)mk[w] * 12 + q * 3 + 1] - Y;
                    const double dist = dx * dx + dy * dy;
                    if (bd < 0 || dist < bd) {
                        bd = dist;
                        best = q;
                    }
                }
                near4[(size_t)i * 4 + w] = mk[w];
                near4[(size_t)i * 4 + 2 + w] = best;
            }
        }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->charuco) {
        // the first board of this context: the tables at their largest, the result slots, the masks -- published when all of it exists
        CharucoBufs *B = new (std::nothrow) CharucoBufs;
        if (!B) return FID_E_OUT_OF_MEMORY;
        const size_t slots = (size_t)c->lim.max_batch + 1;
        MemLayout l;
        l.add(&B->d_ids, CH_MAX_MARKERS), l.add(&B->d_mobj, 12 * CH_MAX_MARKERS), l.add(&B->d_near, 4 * CH_MAX_CORNERS), l.add(&B->d_cobj, 3 * CH_MAX_CORNERS);
        l.add(&B->d_mask, CH_MASK_STRIDE * CH_MAXWIN), l.add(&B->d_n, slots), l.add(&B->d_corners, CH_MAX_CORNERS * slots), l.add(&B->d_bposes, slots);
        l.add(&B->d_cposes, slots);
        const std::vector<float> mask = charuco_subpix_masks();
        hipError_t e = B->mem.reserve(l.bytes());
        if (e == hipSuccess) {
            l.bind(B->mem.p);
            e = hipMemcpy(B->d_mask, mask.data(), mask.size() * sizeof(float), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) delete B;
        HIPCHK(c, e);
        c->charuco = B;
    }
    CharucoBufs *B = c->charuco;
    B->nm = B->nc = 0;
    HIPCHK(c, hipMemcpy(B->d_ids, ids.data(), sizeof(int) * (size_t)nm, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(B->d_mobj, mobj.data(), sizeof(double) * 12 * (size_t)nm, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(B->d_near, near4.data(), sizeof(int) * 4 * (size_t)nc, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(B->d_cobj, cobj.data(), sizeof(double) * 3 * (size_t)nc, hipMemcpyHostToDevice));
    B->board = *board;
    B->nm = nm;
    B->nc = nc;
    return FID_OK;
}

// where one run of the kernels reads and writes
struct ChRun {
    const fid_marker *d_markers;
    const int *d_nmark;
    int nmark_stride_ints, per_frame, F;
    const uint8_t *gray;
    long long gfstride;
    int gs, W, H;
    int slot0;  // the first result slot: 0 for the frames of the last call, max_batch for input from the host
};

// k_charuco_interp (behind k_map_pose on the board's tables, with a camera) and k_charuco_subpix for R.F frames on the context's stream
static fid_status charuco_enqueue(fid_ctx *c, const fid_camera *camera, int min_markers, const ChRun &R)
{
    CharucoBufs *B = c->charuco;
    const ChBoardDev bd = {B->d_near, B->d_mobj, B->d_cobj, B->nm, B->nc, B->board.first_id};
    fid_charuco_corner *d_out = B->d_corners + (size_t)R.slot0 * B->nc;
    int *d_n = B->d_n + R.slot0;
    if (camera) {
        const PoseCam cam = pose_cam_from(*camera, 0.);
        fid_map_pose_out *d_bp = B->d_bposes + R.slot0;
        POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_map_pose<CAM_MODEL>, dim3(R.F), dim3(64), 0, c->stream, R.d_markers, R.d_nmark, R.nmark_stride_ints,
                                                        R.per_frame, (const int *)B->d_ids, (const double *)B->d_mobj, B->nm, cam, d_bp));
        HIPCHK(c, hipGetLastError());
        POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_charuco_interp<CAM_MODEL>, dim3(R.F), dim3(64), 0, c->stream, R.d_markers, R.d_nmark,
                                                        R.nmark_stride_ints, R.per_frame, bd, cam, (const fid_map_pose_out *)d_bp, R.W, R.H, min_markers, d_out,
                                                        B->nc, d_n));
    } else {
        PoseCam cam = {};
        hipLaunchKernelGGL(k_charuco_interp<-1>, dim3(R.F), dim3(64), 0, c->stream, R.d_markers, R.d_nmark, R.nmark_stride_ints, R.per_frame, bd, cam,
                           (const fid_map_pose_out *)nullptr, R.W, R.H, min_markers, d_out, B->nc, d_n);
    }
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_charuco_subpix, dim3(B->nc, R.F), dim3(64), 0, c->stream, R.gray, R.gfstride, R.gs, R.W, R.H, d_out, B->nc, (const int *)d_n,
                       (const float *)B->d_mask);
    HIPCHK(c, hipGetLastError());
    return FID_OK;
}

static void charuco_pose_enqueue(fid_ctx *c, const fid_camera &camera, int slot0, int F)
{
    CharucoBufs *B = c->charuco;
    const PoseCam cam = pose_cam_from(camera, 0.);
    POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_charuco_pose<CAM_MODEL>, dim3(F), dim3(64), 0, c->stream,
                                                    (const fid_charuco_corner *)(B->d_corners + (size_t)slot0 * B->nc), B->nc, (const int *)(B->d_n + slot0),
                                                    (const double *)B->d_cobj, B->nc, B->board.squares_x - 1, cam, B->d_cposes + slot0));
}

static bool charuco_common_refusals(fid_ctx *c, const fid_camera *camera, bool camera_required, int min_markers)
{
    if (camera ? !fid_camera_usable(camera) : camera_required) {
        c->last_error = "ChArUco: a camera that is not usable (or none where one is required)";
        return true;
    }
    if (min_markers < 1 || min_markers > 2) {
        c->last_error = "ChArUco: min_markers " + std::to_string(min_markers) + " is outside 1 .. 2";
        return true;
    }
    return refuse_in_flight(c) || refuse_no_board(c);
}

// the frames of the last call as a ChRun
static ChRun charuco_last_frames(fid_ctx *c)
{
    return {c->d_markers, &c->d_counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), c->P.maxMarkers, c->last_frames, c->last_gray, c->last_gfstride,
            c->P.gstride, c->last_W, c->last_H, 0};
}

// the counts and corners of F frames from slot0 on, into out (cap records a frame): FID_E_CAPACITY where a frame holds more
static fid_status charuco_fetch(fid_ctx *c, int slot0, int F, fid_charuco_corner *out, int cap, int32_t *n_per_frame)
{
    CharucoBufs *B = c->charuco;
    B->h_n.resize((size_t)F);
    B->h_corners.resize((size_t)F * B->nc);
    HIPCHK(c, hipMemcpyAsync(B->h_n.data(), B->d_n + slot0, sizeof(int) * (size_t)F, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(B->h_corners.data(), B->d_corners + (size_t)slot0 * B->nc, sizeof(fid_charuco_corner) * (size_t)F * B->nc,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fid_status rc = FID_OK;
    for (int f = 0; f < F; f++) {
        const int n = B->h_n[(size_t)f];
        n_per_frame[f] = n;
        if (n > cap) {
            c->last_error = "caller room for " + std::to_string(cap) + " ChArUco corners a frame, frame " + std::to_string(f) + " has " + std::to_string(n);
            rc = FID_E_CAPACITY;
        }
        const int m = n < cap ? n : cap;
        if (m > 0) memcpy(out + (size_t)f * cap, B->h_corners.data() + (size_t)f * B->nc, sizeof(fid_charuco_corner) * (size_t)m);
    }
    return rc;
}

fid_status fid_charuco_last_cam(fid_ctx *c, const fid_camera *camera, int32_t min_markers, fid_charuco_corner *out, int32_t cap_per_frame,
                                int32_t *n_per_frame)
{
    if (!c || !n_per_frame || cap_per_frame < 0 || (cap_per_frame > 0 && !out) || c->last_frames <= 0) return FID_E_INVALID_ARG;
    if (charuco_common_refusals(c, camera, false, min_markers)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const fid_status rc = charuco_enqueue(c, camera, min_markers, charuco_last_frames(c));
    if (rc != FID_OK) return rc;
    return charuco_fetch(c, 0, c->last_frames, out, cap_per_frame, n_per_frame);
}

fid_status fid_charuco_interpolate_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, int32_t n, const uint8_t *img, int32_t width,
                                       int32_t height, int32_t stride_bytes, int32_t min_markers, fid_charuco_corner *out, int32_t cap, int32_t *n_out)
{
    if (!c || !n_out || cap < 0 || (cap > 0 && !out) || n < 0 || (n > 0 && !markers) || !img) return FID_E_INVALID_ARG;
    if (width < 8 || height < 8 || stride_bytes < width || width > c->lim.max_width || height > c->lim.max_height) {
        c->last_error = "ChArUco: an image of " + std::to_string(width) + " x " + std::to_string(height) + " (stride " + std::to_string(stride_bytes) +
                        ") is outside the context's frame limits";
        return FID_E_INVALID_ARG;
    }
    if (charuco_common_refusals(c, camera, false, min_markers)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    CharucoBufs *B = c->charuco;
    int *d_n = nullptr;
    fid_status rcs = stage_gray(c, B->img, img, width, height, stride_bytes);
    if (rcs == FID_OK) rcs = stage_markers(c, B->in, markers, n, &d_n);
    if (rcs != FID_OK) return rcs;
    const int slot = c->lim.max_batch;
    const ChRun R = {B->in.markers(), d_n, 0, n > 0 ? n : 1, 1, B->img.data(), 0, width, width, height, slot};
    const fid_status rc = charuco_enqueue(c, camera, min_markers, R);
    if (rc != FID_OK) return rc;
    return charuco_fetch(c, slot, 1, out, cap, n_out);
}

fid_status fid_charuco_pose_last_cam(fid_ctx *c, const fid_camera *camera, int32_t min_markers, fid_charuco_pose_out *out, int32_t cap_frames)
{
    if (!c || !out || c->last_frames <= 0) return FID_E_INVALID_ARG;
    if (charuco_common_refusals(c, camera, true, min_markers)) return FID_E_INVALID_ARG;
    if (refuse_room(c, cap_frames)) return FID_E_CAPACITY;
    HIPCHK(c, hipSetDevice(c->device));
    const fid_status rc = charuco_enqueue(c, camera, min_markers, charuco_last_frames(c));
    if (rc != FID_OK) return rc;
    charuco_pose_enqueue(c, *camera, 0, c->last_frames);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->charuco->d_cposes, sizeof(fid_charuco_pose_out) * (size_t)c->last_frames, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FID_OK;
}

fid_status fid_charuco_pose_cam(fid_ctx *c, const fid_camera *camera, const float *xy, const int32_t *ids, int32_t n, fid_charuco_pose_out *out)
{
    if (!c || !out || n < 0 || (n > 0 && (!xy || !ids))) return FID_E_INVALID_ARG;
    if (charuco_common_refusals(c, camera, true, 1)) return FID_E_INVALID_ARG;
    CharucoBufs *B = c->charuco;
    if (n > B->nc) {
        c->last_error = "ChArUco pose: " + std::to_string(n) + " corners, the board has " + std::to_string(B->nc);
        return FID_E_INVALID_ARG;
    }
    std::vector<fid_charuco_corner> rec((size_t)n);
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= B->nc) {
            c->last_error = "ChArUco pose: corner id " + std::to_string(ids[i]) + " is outside the board's 0 .. " + std::to_string(B->nc - 1);
            return FID_E_INVALID_ARG;
        }
        rec[(size_t)i] = {ids[i], 0, xy[2 * i], xy[2 * i + 1], xy[2 * i], xy[2 * i + 1]};
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int slot = c->lim.max_batch;
    if (n > 0)
        HIPCHK(c, hipMemcpyAsync(B->d_corners + (size_t)slot * B->nc, rec.data(), sizeof(fid_charuco_corner) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(B->d_n + slot, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (rec and n are temporaries)
    charuco_pose_enqueue(c, *camera, slot, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, B->d_cposes + slot, sizeof(fid_charuco_pose_out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FID_OK;
}
