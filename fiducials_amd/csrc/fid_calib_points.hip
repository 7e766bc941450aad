// fid_calib_points.hip -- camera calibration from ChArUco corners (fid_abi.h: "camera calibration from ChArUco corners").  Part of the
// fid_api.hip translation unit, behind fid_charuco.hip.  The point route through fid_calib.hip's solve: a view is a list of chessboard
// corner records instead of a list of markers, and the kernels read its residuals from a table of points instead of from the markers and
// the map.  The Levenberg-Marquardt machine, the residual function, the stop, std_dev and the host steps are fid_calib.hip's
// (cal_view_blocks / cal_view_eval over the source CalPoints, k_calib_solve and k_calib_accept as they are, calib_solve_views).
//   k_calib_start_pts  a wave per view, once: the gather -- the records in list order, an id listed twice left out altogether -- into the
//                      view's point table (object point as three doubles, image point as two floats) and, compacted, into the records
//                      k_charuco_pose takes; the exact test for "all on one line of the grid"; with START_AUTO the plane frame, the DLT
//                      homography to the float pixels and the view's two focal constraints, in k_calib_start's arithmetic.
//   k_charuco_pose     (fid_charuco.hip) a wave per view: the start pose over the view's used points under the start camera.
//   k_calib_init_pts   k_calib_init over fid_charuco_pose_out records.
//   k_calib_blocks_pts, k_calib_eval_pts   K22 and K24 over the point table.
// Nothing of it exists on a context until the first fid_calibrate_charuco.

#define CALP_STRIDE CH_MAX_CORNERS  // rows of a view's point table: a board has at most this many corners, and an id is used once

struct CalPoint {
    double X[3];  // the board's chessboard corner
    float uv[2];  // the refined position
};
static_assert(sizeof(CalPoint) == 32, "CalPoint: a row of the point table");

// residual r of a view is coordinate r & 1 of row r >> 1 of its table
struct CalPoints {
    static constexpr int PER_ITEM = 1;
    const CalPoint *__restrict__ pts;
    const CalPoint *tab;
    __device__ __forceinline__ void bind(int v, const CalCfg *__restrict__) { tab = pts + (size_t)v * CALP_STRIDE; }
    __device__ __forceinline__ void object(int r, double M[3]) const
    {
        const CalPoint *p = tab + (r >> 1);
        M[0] = p->X[0];
        M[1] = p->X[1];
        M[2] = p->X[2];
    }
    __device__ __forceinline__ double image(int r) const { return (double)tab[r >> 1].uv[r & 1]; }
};

struct CalStartPtsLds {
    ChPoseLds p;
    int lst[CALP_STRIDE];  // the used records' list positions, then their ids
    unsigned seen[CH_MAX_CORNERS / 32], dup[CH_MAX_CORNERS / 32];
};

// vinfo[4 v + ..]: 0 n_used, 1 0 (nothing is ever over: an id is used once), 2 the view's status (k_calib_init_pts), 3 bit 1: the
// homography exists, bit 2: the used points lie on one line of the grid.  con: as k_calib_start.  n_posed[v]: the count k_charuco_pose
// gets -- 0 for a view with fewer than min_points used points, which is not posed.
// (the upper bound of the workgroup size is never launched: it keeps the register allocation at k_calib_start's, fid_kernels.hip
// WALKER_WG_ATTR)
__global__ WALKER_WG_ATTR(64, 1024) void k_calib_start_pts(const fid_charuco_corner *__restrict__ corners, const int *__restrict__ n_per_view, int per_view,
                                                         const double *__restrict__ cobj, int nc, int row_len, int min_points, int want_auto, double cx0,
                                                         double cy0, CalPoint *__restrict__ pts, fid_charuco_corner *__restrict__ used,
                                                         int *__restrict__ n_posed, int *__restrict__ vinfo, double *__restrict__ con)
{
    __shared__ CalStartPtsLds s;
    const int v = blockIdx.x, lane = threadIdx.x;
    const fid_charuco_corner *src = corners + (long long)v * per_view;
    int nm = n_per_view[v];
    nm = nm < 0 ? 0 : (nm > per_view ? per_view : nm);
    nc = nc > CH_MAX_CORNERS ? CH_MAX_CORNERS : nc;
    // ---- the gather: a bit per corner id that is listed, a second bit where it is listed again; then the survivors in list order
    for (int e = lane; e < CH_MAX_CORNERS / 32; e += 64) s.seen[e] = s.dup[e] = 0u;
    SR_LDS_SYNC();
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        const int id = m < nm ? src[m].id : -1;
        if (id >= 0 && id < nc) {
            const unsigned bit = 1u << (id & 31);
            if (atomicOr(&s.seen[id >> 5], bit) & bit) atomicOr(&s.dup[id >> 5], bit);
        }
    }
    SR_LDS_SYNC();
    int found = 0;
    for (int m0 = 0; m0 < nm; m0 += 64) {
        const int m = m0 + lane;
        const int id = m < nm ? src[m].id : -1;
        const bool keep = id >= 0 && id < nc && !(s.dup[id >> 5] >> (id & 31) & 1u);
        const unsigned long long hit = __ballot(keep);
        if (keep) {
            const int pos = found + __builtin_popcountll(hit & ((1ull << lane) - 1ull));
            if (pos < CALP_STRIDE) s.lst[pos] = m;
        }
        found += __builtin_popcountll(hit);
    }
    found = found > CALP_STRIDE ? CALP_STRIDE : found;  // (cannot happen: every kept id is listed once and there are nc <= CALP_STRIDE ids)
    SR_LDS_SYNC();
    // ---- the view's point table, the compacted records, the points for the homography
    for (int k = lane; k < found; k += 64) {
        const fid_charuco_corner rec = src[s.lst[k]];
        CalPoint P;
        for (int a = 0; a < 3; a++) P.X[a] = cobj[3 * (size_t)rec.id + a];
        P.uv[0] = rec.x;
        P.uv[1] = rec.y;
        pts[(size_t)v * CALP_STRIDE + k] = P;
        used[(size_t)v * CALP_STRIDE + k] = rec;
        s.p.obj[k][0] = P.X[0];
        s.p.obj[k][1] = P.X[1];
        s.p.mn[k][0] = rec.x;  // (findHomography's input is float: the positions as they are)
        s.p.mn[k][1] = rec.y;
        s.lst[k] = rec.id;
    }
    SR_LDS_SYNC();
    // ---- all on one line of the grid?  k_charuco_pose's test: exactly, on the integer (cx, cy)
    bool one_line = true;
    if (found > 0) {
        const int x0 = s.lst[0] % row_len, y0 = s.lst[0] / row_len;
        int first = found;
        for (int p = lane; p < found; p += 64) {
            const int id = s.lst[p];
            if ((id % row_len != x0 || id / row_len != y0) && p < first) first = p;
        }
        for (int mask = 1; mask < 64; mask <<= 1) {
            const int o = __shfl_xor(first, mask, WAVE);
            first = o < first ? o : first;
        }
        bool off_line = false;
        if (first < found) {
            const int dx = s.lst[first] % row_len - x0, dy = s.lst[first] / row_len - y0;
            for (int p = lane; p < found; p += 64) {
                const int id = s.lst[p];
                off_line = off_line || dx * (id / row_len - y0) - dy * (id % row_len - x0) != 0;
            }
        }
        one_line = __ballot(off_line) == 0ull;
    }
    int flags = one_line ? 4 : 0;
    double c6[6] = {0, 0, 0, 0, 0, 0};
    if (want_auto && found >= min_points && !one_line) {
        // ---- k_calib_start's plane frame and homography (the board's z is 0: the sums over it are left out, they are exactly 0)
        const int n = found;
        double Mc[3] = {0, 0, 0}, W[3], Vt[3][3];
        for (int p = lane; p < n; p += 64) {
            Mc[0] += s.p.obj[p][0];
            Mc[1] += s.p.obj[p][1];
        }
        for (int a = 0; a < 2; a++) Mc[a] = wave_sum_f64(Mc[a]) / n;
        double m3[3] = {0, 0, 0};
        for (int p = lane; p < n; p += 64) {
            const double d0 = s.p.obj[p][0] - Mc[0], d1 = s.p.obj[p][1] - Mc[1];
            m3[0] += d0 * d0; m3[1] += d0 * d1; m3[2] += d1 * d1;
        }
        for (int i = 0; i < 3; i++) m3[i] = wave_sum_f64(m3[i]);
        double MM[3][3] = {{m3[0], m3[1], 0.}, {m3[1], m3[2], 0.}, {0., 0., 0.}};
        pnp_scatter_eig(MM, W, Vt);
        if (W[2] / W[1] < 1e-3) {
            double Rt[9], tt[3], h[9];
            pnp_plane_frame(Vt, Mc, Rt, tt);
            for (int p = lane; p < n; p += 64) {
                s.p.Mxy[p][0] = (float)(Rt[0] * s.p.obj[p][0] + Rt[1] * s.p.obj[p][1] + tt[0]);
                s.p.Mxy[p][1] = (float)(Rt[3] * s.p.obj[p][0] + Rt[4] * s.p.obj[p][1] + tt[1]);
            }
            SR_LDS_SYNC();
            if (pnp_homography_dlt(ChPoseView{&s.p}, n, lane, h) && cal_focal_rows(h, cx0, cy0, c6)) flags |= 2;
        }
    }
    if (lane == 0) {
        vinfo[4 * v] = found;
        vinfo[4 * v + 1] = 0;
        vinfo[4 * v + 2] = 0;
        vinfo[4 * v + 3] = flags;
        n_posed[v] = found >= min_points ? found : 0;
        for (int j = 0; j < 6; j++) con[6 * v + j] = (flags & 2) ? c6[j] : 0.;
    }
}

__global__ __launch_bounds__(64) void k_calib_init_pts(const CalCfg *__restrict__ cfg, CalState *__restrict__ st, int *__restrict__ vinfo,
                                                        const fid_charuco_pose_out *__restrict__ vpose, double *__restrict__ pose)
{
    cal_init_views(cfg, st, vinfo, vpose, pose, [](const fid_charuco_pose_out *o) { return o->status == FID_CHARUCO_POSE_OK; });
}

template <int MODEL>
__global__ WALKER_WG_ATTR(64, 1024) void k_calib_blocks_pts(const CalCfg *__restrict__ cfg, const CalState *__restrict__ st, const CalPoint *__restrict__ pts,
                                                          const int *__restrict__ vinfo, const double *__restrict__ pose, double *__restrict__ blk,
                                                          double *__restrict__ sch, double *__restrict__ cost, int final)
{
    cal_view_blocks<MODEL>(cfg, st, CalPoints{pts, nullptr}, vinfo, pose, blk, sch, cost, final);
}

template <int MODEL>
__global__ __launch_bounds__(64) void k_calib_eval_pts(const CalCfg *__restrict__ cfg, const CalState *__restrict__ st, const CalPoint *__restrict__ pts,
                                                        const int *__restrict__ vinfo, const double *__restrict__ pose, const double *__restrict__ blk,
                                                        double *__restrict__ cand_pose, double *__restrict__ cand_cost, double *__restrict__ dnpn)
{
    cal_view_eval<MODEL>(cfg, st, CalPoints{pts, nullptr}, vinfo, pose, blk, cand_pose, cand_cost, dnpn);
}

// ------------------------------------------------------------------------------------------------ host
// what the point route needs beside fid_calib.hip's CalibBufs: the caller's records, and per view the point table, the compacted
// records, the count and the record of k_charuco_pose
struct CalibPtsBufs {
    int cap_views = 0;
    DevArray<fid_charuco_corner> in;
    DevBlock mem;  // everything below, sized by cap_views
    CalPoint *d_pts = nullptr;
    fid_charuco_corner *d_used = nullptr;
    int *d_nposed = nullptr;
    fid_charuco_pose_out *d_vpose = nullptr;
};

static void calib_pts_free(fid_ctx *c)
{
    delete c->calib_pts;
    c->calib_pts = nullptr;
}

static fid_status calib_pts_ensure(fid_ctx *c, int n_views, size_t n_in)
{
    if (!c->calib_pts) c->calib_pts = new (std::nothrow) CalibPtsBufs();
    CalibPtsBufs *p = c->calib_pts;
    if (!p) return FID_E_OUT_OF_MEMORY;
    HIPCHK(c, p->in.reserve(n_in));
    if (n_views > p->cap_views) {
        p->cap_views = 0;
        const size_t V = (size_t)n_views;
        MemLayout l;
        l.add(&p->d_pts, CALP_STRIDE * V), l.add(&p->d_used, CALP_STRIDE * V), l.add(&p->d_nposed, V), l.add(&p->d_vpose, V);
        HIPCHK(c, p->mem.reserve(l.bytes()));
        l.bind(p->mem.p);
        p->cap_views = n_views;
    }
    return FID_OK;
}

fid_status fid_calibrate_charuco(fid_ctx *c, const fid_charuco_corner *corners, const int32_t *n_per_view, int32_t n_views, int32_t cap_per_view,
                                 int32_t image_w, int32_t image_h, const fid_calib_opts *opts, fid_camera *cam_io, fid_calib_out *out, fid_calib_view *views)
{
    static const char who[] = "fid_calibrate_charuco";
    if (!c) return FID_E_INVALID_ARG;
    if (calib_refuse_args(c, who, corners, n_per_view, n_views, cap_per_view, image_w, image_h, opts, cam_io, out)) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_board(c)) return FID_E_INVALID_ARG;
    fid_camera start = fid_camera_normalised(*cam_io);
    if (calib_refuse_start(c, who, opts, start)) return FID_E_INVALID_ARG;
    CharucoBufs *B = c->charuco;
    for (int v = 0; v < n_views; v++) {
        const int n = n_per_view[v] < 0 ? 0 : (n_per_view[v] > cap_per_view ? cap_per_view : n_per_view[v]);
        const fid_charuco_corner *r = corners + (size_t)v * cap_per_view;
        for (int i = 0; i < n; i++) {
            if (r[i].id < 0 || r[i].id >= B->nc)
                return calib_refuse(c, who, "view " + std::to_string(v) + ", record " + std::to_string(i) + ": corner id " + std::to_string(r[i].id) +
                                                " is outside the board's 0 .. " + std::to_string(B->nc - 1)),
                       FID_E_INVALID_ARG;
            if (r[i].x - r[i].x != 0.f || r[i].y - r[i].y != 0.f)
                return calib_refuse(c, who, "view " + std::to_string(v) + ", record " + std::to_string(i) + ": a coordinate is not finite"), FID_E_INVALID_ARG;
        }
    }
    unsigned mask = 0;
    const int min_points = opts->min_markers > 4 ? opts->min_markers : 4;
    const CalCfg cfg = calib_config(opts, start, n_views, cap_per_view, 1, min_points, &mask);

    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_in = (size_t)n_views * cap_per_view;
    fid_status rce = calib_ensure(c, n_views, 0);
    if (rce == FID_OK) rce = calib_pts_ensure(c, n_views, n_in);
    if (rce != FID_OK) return rce;
    CalibBufs *b = c->calib;
    CalibPtsBufs *p = c->calib_pts;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(p->in.data(), corners, sizeof(fid_charuco_corner) * n_in, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(b->d_n, n_per_view, sizeof(int) * (size_t)n_views, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(b->mem.p + b->zero_from, 0, b->zero_bytes, st));
    // ---- the views' used points; with AUTO the focal constraints
    const double cx0 = (mask >> 2 & 1u) ? 0.5 * (image_w - 1) : start.K[2], cy0 = (mask >> 3 & 1u) ? 0.5 * (image_h - 1) : start.K[5];
    const int row_len = B->board.squares_x - 1;
    hipLaunchKernelGGL(k_calib_start_pts, dim3(n_views), dim3(64), 0, st, (const fid_charuco_corner *)p->in.data(), (const int *)b->d_n, cap_per_view,
                       (const double *)B->d_cobj, B->nc, row_len, min_points, cfg.start_auto, cx0, cy0, p->d_pts, p->d_used, p->d_nposed, b->d_vinfo, b->d_con);
    HIPCHK(c, hipGetLastError());
    if (cfg.start_auto) {
        const fid_status rca = calib_auto_start(c, who, cfg, mask, cx0, cy0, false, &start);
        if (rca != FID_OK) return rca;
    }
    if (cfg.fix_aspect) start.K[0] = cfg.aspect * start.K[4];
    // ---- the start poses: k_charuco_pose over the views' used points under the start camera
    const PoseCam cam = pose_cam_from(start, 0.);
    const int model = start.model;
    POSE_CAM_DISPATCH(model, hipLaunchKernelGGL(k_charuco_pose<CAM_MODEL>, dim3(n_views), dim3(64), 0, st, (const fid_charuco_corner *)p->d_used, CALP_STRIDE,
                                                (const int *)p->d_nposed, (const double *)B->d_cobj, B->nc, row_len, cam, p->d_vpose));
    HIPCHK(c, hipGetLastError());
    return calib_solve_views(
        c, who, "no view can be used (too few corners, all on one line of the grid, or no start pose)", cfg, mask, start,
        [&] {
            hipLaunchKernelGGL(k_calib_init_pts, dim3(1), dim3(64), 0, st, (const CalCfg *)b->d_cfg, b->d_state, b->d_vinfo,
                               (const fid_charuco_pose_out *)p->d_vpose, b->d_pose);
        },
        [&](int final) {
            POSE_CAM_DISPATCH(model, hipLaunchKernelGGL(k_calib_blocks_pts<CAM_MODEL>, dim3(n_views), dim3(64), 0, st, (const CalCfg *)b->d_cfg,
                                                        (const CalState *)b->d_state, (const CalPoint *)p->d_pts, (const int *)b->d_vinfo,
                                                        (const double *)b->d_pose, b->d_blk, b->d_sch, b->d_cost, final));
        },
        [&] {
            POSE_CAM_DISPATCH(model, hipLaunchKernelGGL(k_calib_eval_pts<CAM_MODEL>, dim3(n_views), dim3(64), 0, st, (const CalCfg *)b->d_cfg,
                                                        (const CalState *)b->d_state, (const CalPoint *)p->d_pts, (const int *)b->d_vinfo,
                                                        (const double *)b->d_pose, (const double *)b->d_blk, b->d_cand, b->d_ccost, b->d_dnpn));
        },
        cam_io, out, views);
}
