// fid_rig_pose.hip -- one rig pose per time step from all cameras of a multi-camera rig (fid_abi.h).  Part of the fid_api.hip
// translation unit, behind fid_map_pose.hip (mp_find, MP_BIT_WORDS) and fid_pnp.h (pnp_wave_solve, LevMarq, pnp_covariance).
//
// ------------------------------------------------------------------------------------------------ K21: rig pose
// One wave per time step (blockIdx.x: the time steps of a batch are one launch).  With C cameras, the step's frames are C marker
// lists: frames step * C .. step * C + C - 1 of the last call, or C lists laid end to end (fid_rig_pose).
//   (1) gather.  Camera by camera, each frame as mp_gather does it (binary search in the map's ids, a bit per entry for "seen" and
//       "seen twice", compaction in list order by ballot and prefix count) into ONE table that goes on over the cameras: a camera's
//       markers are contiguous (first[c] .. first[c + 1]).  An equidistant camera's marker with a corner beyond the model is dropped
//       here and counted, before the cut at RG_MAX_USED.  Then the points: the map's object points, the image points widened, the
//       camera of every point, the undistorted point rounded to float and the marker's image area.
//   (2) start.  The camera with the largest summed marker area; pnp_wave_solve<its model> on a view of its rows of the tables, as
//       k_map_pose would pose that frame; composed with the camera's extrinsic to the rig's start.
//   (3) joint solve.  LevMarq over the 2 N residuals of all cameras: residual r on lane r % 64, per-lane partial sums in residual
//       order, one xor butterfly.  rvec -> R and dR/dr once per evaluation; per residual the point goes through (R, t), through its
//       camera's (R_c, t_c) and through project_one<its model> at the identity pose, whose d/d tvec IS the gradient with respect
//       to the camera-frame point: Jrow = (R_c^T g) . [dR/dr_i M, I].  The model is a run-time switch per point, so cameras of
//       different models share a rig; project_one's instantiations for the other kernels are what they were.
//   (4) the record: the reprojection error over all points and per camera, and with cov the covariance from J^T J at the result.
// LDS (RgLds, 42 072 B static): 12 KB object points + 8 KB image points + 8 KB of float pairs (mn, Mxy) + 4 KB of squared errors (512
// points each) + 2.3 KB for the DLT (A, V, the marker areas) + the 4.3 KB camera table (16 x 272 B) + 512 B of per-point camera indices
// + 2.1 KB of tables (mk, ent, seen, dup, first).

#define RG_MAX_USED FID_RIG_MAX_USED
#define RG_MAX_PTS (4 * RG_MAX_USED)
#define RG_CAM_WORDS (sizeof(fid_rig_camera) / 8)
static_assert(sizeof(fid_rig_camera) % 8 == 0, "fid_rig_camera is copied as 8-byte words");
struct RgLds {
    double obj[RG_MAX_PTS][3], img[RG_MAX_PTS][2];
    float mn[RG_MAX_PTS][2], Mxy[RG_MAX_PTS][2];
    double e2[RG_MAX_PTS];
    double A[81], V[81], area[RG_MAX_USED];
    fid_rig_camera cams[FID_RIG_MAX_CAMERAS];
    int mk[RG_MAX_USED], ent[RG_MAX_USED];
    unsigned seen[MP_BIT_WORDS], dup[MP_BIT_WORDS];
    int first[FID_RIG_MAX_CAMERAS + 1];
    unsigned char pcam[RG_MAX_PTS];
};
static_assert(sizeof(RgLds) <= 64 * 1024, "k_rig_pose: static LDS");

// pnp_undistort of the camera's model, chosen at run time
__device__ __forceinline__ bool rg_undistort(const fid_camera &cam, double u, double v, double *x, double *y)
{
    switch (cam.model) {
    case FID_CAM_RATIONAL: return pnp_undistort<FID_CAM_RATIONAL>(cam.K, cam.D, u, v, x, y);
    case FID_CAM_EQUIDISTANT: return pnp_undistort<FID_CAM_EQUIDISTANT>(cam.K, cam.D, u, v, x, y);
    default: return pnp_undistort<FID_CAM_PLUMB_BOB>(cam.K, cam.D, u, v, x, y);
    }
}

// coordinate sel of the camera-frame point Xc under the camera's model, with g = d / d Xc: project_one at the identity pose, where
// the point it projects is Xc itself and its d / d tvec is the gradient asked for
__device__ __forceinline__ double rg_cam_project(const fid_camera &cam, const double Xc[3], int sel, double g[3], bool wantJ)
{
    const double ident[6] = {0., 0., 0., 0., 0., 0.};
    double Jrow[6], out;
    switch (cam.model) {
    case FID_CAM_RATIONAL: out = project_one<FID_CAM_RATIONAL>(Xc, ident, cam.K, cam.D, sel, Jrow, wantJ); break;
    case FID_CAM_EQUIDISTANT: out = project_one<FID_CAM_EQUIDISTANT>(Xc, ident, cam.K, cam.D, sel, Jrow, wantJ); break;
    default: out = project_one<FID_CAM_PLUMB_BOB>(Xc, ident, cam.K, cam.D, sel, Jrow, wantJ); break;
    }
    if (wantJ)
        for (int a = 0; a < 3; a++) g[a] = Jrow[3 + a];
    return out;
}

// coordinate sel of point p of the tables through the rig pose (R = R(rvec) with dRdr, t) and its camera; Jrow = d / d (rvec, tvec)
__device__ __forceinline__ double rg_project(const RgLds &s, int p, const double R[9], const double dRdr[27], const double t[3], int sel, double Jrow[6],
                                             bool wantJ)
{
    const fid_rig_camera &rc = s.cams[s.pcam[p]];
    const double M[3] = {s.obj[p][0], s.obj[p][1], s.obj[p][2]};
    double Xr[3], Xc[3], g[3];
    for (int a = 0; a < 3; a++) Xr[a] = R[3 * a] * M[0] + R[3 * a + 1] * M[1] + R[3 * a + 2] * M[2] + t[a];
    for (int a = 0; a < 3; a++) Xc[a] = rc.R[3 * a] * Xr[0] + rc.R[3 * a + 1] * Xr[1] + rc.R[3 * a + 2] * Xr[2] + rc.t[a];
    const double out = rg_cam_project(rc.cam, Xc, sel, g, wantJ);
    if (wantJ) {
        double h[3];  // R_c^T g
        for (int j = 0; j < 3; j++) h[j] = rc.R[j] * g[0] + rc.R[3 + j] * g[1] + rc.R[6 + j] * g[2];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double *dR = dRdr + 9 * i;
            const double d0 = dR[0] * M[0] + dR[1] * M[1] + dR[2] * M[2];
            const double d1 = dR[3] * M[0] + dR[4] * M[1] + dR[5] * M[2];
            const double d2 = dR[6] * M[0] + dR[7] * M[1] + dR[8] * M[2];
            Jrow[i] = h[0] * d0 + h[1] * d1 + h[2] * d2;
            Jrow[3 + i] = h[i];
        }
    }
    return out;
}

// pnp_wave_residuals over all n points of the tables, each through its own camera: the lane's share of |e|^2; with needJ S = J^T J and,
// with GRAD, gJ = J^T e, the same in every lane
template <bool GRAD>
__device__ __forceinline__ double rg_wave_residuals(const RgLds &s, int n, int lane, const double param[6], bool needJ, double S[21], double gJ[6])
{
    double R[9], dRdr[27];
    rodrigues_v2m(param, R, dRdr, needJ);
    const int nres = 2 * n;
    double Sp[21], gp[6], e2 = 0;
    for (int i = 0; i < 21; i++) Sp[i] = 0.;
    for (int i = 0; i < 6; i++) gp[i] = 0.;
    for (int r = lane; r < nres; r += 64) {
        const int p = r >> 1, sel = r & 1;
        double Jrow[6];
        const double err = rg_project(s, p, R, dRdr, param + 3, sel, Jrow, needJ) - s.img[p][sel];
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

// fid_pnp.h's view of ONE camera's rows of the tables: points p0 .. p0 + n, markers k0 .. k0 + nmk
struct RgCamView {
    RgLds *s;
    int p0, k0, nmk;
    static constexpr bool PLANAR_ONLY = false;
    __device__ __forceinline__ void obj(int i, double M[3]) const
    {
        for (int a = 0; a < 3; a++) M[a] = s->obj[p0 + i][a];
    }
    __device__ __forceinline__ double img(int i, int c) const { return s->img[p0 + i][c]; }
    __device__ __forceinline__ float mn(int i, int c) const { return s->mn[p0 + i][c]; }
    __device__ __forceinline__ float *Mxy(int i) const { return s->Mxy[p0 + i]; }
    __device__ __forceinline__ double *A() const { return s->A; }
    __device__ __forceinline__ double *V() const { return s->V; }
    __device__ __forceinline__ int markers() const { return nmk; }
    __device__ __forceinline__ double area(int k) const { return s->area[k0 + k]; }
    static constexpr bool MARKER_IN_PLACE = false;
    __device__ __forceinline__ int first(int k) const { return 4 * k; }
};

// per_frame > 0: camera c of step `step` reads frame f = step * C + c: markers + f * per_frame, nmark[f * nmark_stride_ints] of them (at
// most per_frame).  per_frame == 0 (one step): the C lists lie end to end in markers, nmark[c] of them for camera c.
__global__ __launch_bounds__(64) void k_rig_pose(const fid_marker *__restrict__ markers, const int *__restrict__ nmark, int nmark_stride_ints, int per_frame,
                                                  const fid_rig_camera *__restrict__ cams, int C, const int *__restrict__ map_ids,
                                                  const double *__restrict__ map_obj, int map_n, fid_rig_pose_out *__restrict__ out, double sigma_px,
                                                  fid_map_pose_cov *__restrict__ cov)
{
    __shared__ RgLds s;
    const int step = blockIdx.x, lane = threadIdx.x;
    C = C < 1 ? 1 : (C > FID_RIG_MAX_CAMERAS ? FID_RIG_MAX_CAMERAS : C);
    map_n = map_n > FID_MAP_MAX_ENTRIES ? FID_MAP_MAX_ENTRIES : map_n;
    for (int e = lane; e < C * (int)RG_CAM_WORDS; e += 64) ((unsigned long long *)s.cams)[e] = ((const unsigned long long *)cams)[e];
    const fid_marker *mbase = markers + (long long)step * C * per_frame;
    // ---- (1) the step's markers that the map names, camera by camera
    int found = 0, n_unposable = 0, off = 0;
    for (int c = 0; c < C; c++) {
        int nm = nmark[((long long)step * C + c) * nmark_stride_ints];
        nm = nm < 0 ? 0 : nm;
        if (per_frame > 0) {
            nm = nm > per_frame ? per_frame : nm;
            off = c * per_frame;
        }
        const fid_marker *mlist = mbase + off;
        if (lane == 0) s.first[c] = found < RG_MAX_USED ? found : RG_MAX_USED;
        for (int e = lane; e < MP_BIT_WORDS; e += 64) s.seen[e] = s.dup[e] = 0u;
        SR_LDS_SYNC();
        const fid_camera &cam = s.cams[c].cam;
        for (int m0 = 0; m0 < nm; m0 += 64) {
            const int m = m0 + lane;
            const int idx = m < nm ? mp_find(map_ids, map_n, mlist[m].id) : -1;
            if (idx >= 0) {
                const unsigned bit = 1u << (idx & 31);
                if (atomicOr(&s.seen[idx >> 5], bit) & bit) atomicOr(&s.dup[idx >> 5], bit);
            }
        }
        SR_LDS_SYNC();
        for (int m0 = 0; m0 < nm; m0 += 64) {
            const int m = m0 + lane;
            int idx = m < nm ? mp_find(map_ids, map_n, mlist[m].id) : -1;
            if (idx >= 0 && (s.dup[idx >> 5] >> (idx & 31) & 1u)) idx = -1;
            bool beyond = false;
            if (idx >= 0 && cam.model == FID_CAM_EQUIDISTANT) {
                for (int q = 0; q < 4; q++) {
                    double x, y;
                    beyond = !rg_undistort(cam, (double)mlist[m].corners[2 * q], (double)mlist[m].corners[2 * q + 1], &x, &y) || beyond;
                }
                if (beyond) idx = -1;
            }
            n_unposable += __builtin_popcountll(__ballot(beyond));
            const unsigned long long hit = __ballot(idx >= 0);
            if (idx >= 0) {
                const int pos = found + __builtin_popcountll(hit & ((1ull << lane) - 1ull));
                if (pos < RG_MAX_USED) {
                    s.mk[pos] = off + m;
                    s.ent[pos] = idx;
                    for (int q = 0; q < 4; q++) s.pcam[4 * pos + q] = (unsigned char)c;
                }
            }
            found += __builtin_popcountll(hit);
        }
        SR_LDS_SYNC();  // (the next camera clears seen / dup)
        if (per_frame == 0) off += nm;
    }
    const int n_over = found > RG_MAX_USED ? found - RG_MAX_USED : 0;
    const int used = found - n_over;
    if (lane == 0) s.first[C] = used;
    if (used == 0) {  // nobody sees the map: the zero record, written as words
        static_assert(sizeof(fid_rig_pose_out) % 8 == 0, "fid_rig_pose_out is zeroed as 8-byte words");
        for (int e = lane; e < (int)(sizeof(fid_rig_pose_out) / 8); e += 64) ((unsigned long long *)(out + step))[e] = 0ull;
        if (cov && lane == 0) pnp_cov_zero(&cov[step].pose, 1, 0, cov[step].cov_cam_pose);
        return;
    }
    SR_LDS_SYNC();
    const int npts = 4 * used;
    for (int p = lane; p < npts; p += 64) {
        const int k = p >> 2, q = p & 3;
        const fid_marker *mk = mbase + s.mk[k];
        const double *src = map_obj + (size_t)s.ent[k] * 12 + q * 3;
        for (int a = 0; a < 3; a++) s.obj[p][a] = src[a];
        const double u = (double)mk->corners[2 * q], v = (double)mk->corners[2 * q + 1];
        s.img[p][0] = u;
        s.img[p][1] = v;
        double x, y;
        (void)rg_undistort(s.cams[s.pcam[p]].cam, u, v, &x, &y);
        s.mn[p][0] = (float)x;
        s.mn[p][1] = (float)y;
        if (q == 0) {  // the marker's area in the image (shoelace over its four corners)
            double a2 = 0;
            for (int i = 0; i < 4; i++) {
                const int i1 = (i + 1) & 3;
                a2 += (double)mk->corners[2 * i] * (double)mk->corners[2 * i1 + 1] - (double)mk->corners[2 * i1] * (double)mk->corners[2 * i + 1];
            }
            s.area[k] = fabs(a2);
        }
    }
    SR_LDS_SYNC();
    // ---- (2) the start camera: the largest summed area, the lowest index of equals (every lane the same sums in the same order)
    int sc = 0, n_cameras = 0;
    double best = -1.;
    for (int c = 0; c < C; c++) {
        const int k0 = s.first[c], k1 = s.first[c + 1];
        if (k1 == k0) continue;
        n_cameras++;
        double a = 0;
        for (int k = k0; k < k1; k++) a += s.area[k];
        if (a > best) {
            best = a;
            sc = c;
        }
    }
    double param[6];
    {
        const fid_rig_camera &rc = s.cams[sc];
        const double *K = rc.cam.K, *kd = rc.cam.D;  // (where they lie in LDS)
        double ps[6], err_s;
        const int k0 = s.first[sc], nmk = s.first[sc + 1] - k0;
        const RgCamView view = {&s, 4 * k0, k0, nmk};
        switch (rc.cam.model) {
        case FID_CAM_RATIONAL: pnp_wave_solve<FID_CAM_RATIONAL>(view, 4 * nmk, lane, K, kd, ps, &err_s); break;
        case FID_CAM_EQUIDISTANT: pnp_wave_solve<FID_CAM_EQUIDISTANT>(view, 4 * nmk, lane, K, kd, ps, &err_s); break;
        default: pnp_wave_solve<FID_CAM_PLUMB_BOB>(view, 4 * nmk, lane, K, kd, ps, &err_s); break;
        }
        // the map in the rig: R = R_c^T R_s, t = R_c^T (t_s - t_c)
        double Rs[9], R0[9], dummy[27];
        rodrigues_v2m(ps, Rs, dummy, false);
        const double d[3] = {ps[3] - rc.t[0], ps[4] - rc.t[1], ps[5] - rc.t[2]};
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) R0[3 * i + j] = rc.R[i] * Rs[j] + rc.R[3 + i] * Rs[3 + j] + rc.R[6 + i] * Rs[6 + j];
            param[3 + i] = rc.R[i] * d[0] + rc.R[3 + i] * d[1] + rc.R[6 + i] * d[2];
        }
        rodrigues_m2v(R0, param);
    }
    // ---- (3) CvLevMarq over the 2 N residuals of all cameras
    {
        double S[21], gJ[6], e2 = 0;
        bool needJ = true;
        LevMarq lm;
        do {
            e2 = rg_wave_residuals<true>(s, npts, lane, param, needJ, S, gJ);
        } while (lm.step(param, S, gJ, [&] { return wave_sum_f64(e2); }, needJ));
    }
    // ---- (4) getReprojectionError over all points and over each camera's (point i of a range on lane i % 64)
    {
        double R[9], dummy[27], Jrow[6];
        rodrigues_v2m(param, R, dummy, false);
        for (int p = lane; p < npts; p += 64) {
            const double dx = s.img[p][0] - (double)(float)rg_project(s, p, R, dummy, param + 3, 0, Jrow, false);
            const double dy = s.img[p][1] - (double)(float)rg_project(s, p, R, dummy, param + 3, 1, Jrow, false);
            const double e = sqrt(dx * dx + dy * dy);
            s.e2[p] = e * e;
        }
    }
    SR_LDS_SYNC();
    double tot = 0;
    for (int p = lane; p < npts; p += 64) tot += s.e2[p];
    const double image_error = wave_sum_f64(tot) / npts;
    if (lane == 0) {
        fid_rig_pose_out o;
#pragma unroll
        for (int c = 0; c < FID_RIG_MAX_CAMERAS; c++) {
            o.n_per_camera[c] = 0;
            o.err_per_camera[c] = 0.;
        }
        o.n_markers = used;
        o.n_cameras = n_cameras;
        o.n_over = n_over;
        o.n_unposable = n_unposable;
        o.start_camera = sc;
        o.reserved0 = 0;
        for (int i = 0; i < 3; i++) {
            o.rvec[i] = param[i];
            o.tvec[i] = param[3 + i];
        }
        double dummy[27];
        rodrigues_v2m(param, o.R, dummy, false);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o.rig_R[3 * i + j] = o.R[3 * j + i];
            o.rig_t[i] = -(o.R[i] * param[3] + o.R[3 + i] * param[4] + o.R[6 + i] * param[5]);
        }
        o.image_error = image_error;
        out[step] = o;
    }
    for (int c = 0; c < C; c++) {  // (the per-camera entries go straight to the record)
        const int p0 = 4 * s.first[c], p1 = 4 * s.first[c + 1];
        if (p1 == p0) continue;
        double tc = 0;
        for (int p = p0 + lane; p < p1; p += 64) tc += s.e2[p];
        tc = wave_sum_f64(tc) / (p1 - p0);
        if (lane == 0) {
            out[step].n_per_camera[c] = (p1 - p0) >> 2;
            out[step].err_per_camera[c] = tc;
        }
    }
    if (cov) {
        // ---- the covariance: J and e at the returned param, summed as the Levenberg-Marquardt sums are
        double S[21];
        const double e2 = wave_sum_f64(rg_wave_residuals<false>(s, npts, lane, param, true, S, nullptr));
        if (lane == 0) pnp_covariance<true>(S, e2, npts, param, sigma_px, &cov[step].pose, cov[step].cov_cam_pose);
    }
}

// ------------------------------------------------------------------------------------------------ host
// everything a rig needs on a context (nothing of it exists until the first fid_set_rig): the camera table, max_batch + 1 records
// and covariances (the slot behind a batch's serves fid_rig_pose), the counts of fid_rig_pose's lists, staging for its markers
struct RigBufs {
    fid_rig_camera *d_cams = nullptr;
    fid_rig_pose_out *d_out = nullptr;
    fid_map_pose_cov *d_cov = nullptr;
    int *d_cnt = nullptr;
    DevBlock mem;  // everything above
    MarkerStage in;
    int n = 0;  // cameras of the rig (0: none set)
};

static void rig_free(fid_ctx *c)
{
    delete c->rig;
    c->rig = nullptr;
}

fid_status fid_rig_camera_from_tf(const double xyz[3], const double quat_xyzw[4], const fid_camera *cam, fid_rig_camera *out)
{
    if (!xyz || !quat_xyzw || !cam || !out) return FID_E_INVALID_ARG;
    double q[4], n2 = 0;
    for (int i = 0; i < 4; i++) {
        q[i] = quat_xyzw[i];
        n2 += q[i] * q[i];
    }
    bool finite = n2 - n2 == 0;
    for (int i = 0; i < 3; i++) finite = finite && xyz[i] - xyz[i] == 0;
    if (!finite || !(n2 > 0.)) return FID_E_INVALID_ARG;
    const double inv = 1. / sqrt(n2);
    const double x = q[0] * inv, y = q[1] * inv, z = q[2] * inv, w = q[3] * inv;
    // the camera in the rig: X_rig = Rq X_cam + xyz
    const double Rq[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                          2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                          2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
    out->cam = *cam;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out->R[3 * i + j] = Rq[3 * j + i];
        out->t[i] = -(Rq[i] * xyz[0] + Rq[3 + i] * xyz[1] + Rq[6 + i] * xyz[2]);
    }
    return FID_OK;
}

fid_status fid_set_rig(fid_ctx *c, const fid_rig_camera *cams, int32_t n)
{
    if (!c || n < 0 || (n > 0 && !cams)) return FID_E_INVALID_ARG;
    if (n > FID_RIG_MAX_CAMERAS) {
        c->last_error = "a rig holds at most " + std::to_string(FID_RIG_MAX_CAMERAS) + " cameras (FID_RIG_MAX_CAMERAS), not " + std::to_string(n);
        return FID_E_UNSUPPORTED;
    }
    if (refuse_in_flight(c)) return FID_E_INVALID_ARG;
    std::vector<fid_rig_camera> tab((size_t)n);
    for (int i = 0; i < n; i++) {
        const fid_rig_camera &rc = cams[i];
        const std::string who = "rig camera " + std::to_string(i) + ": ";
        if (!fid_camera_usable(&rc.cam)) {
            c->last_error = who + "model " + std::to_string(rc.cam.model) + " with " + std::to_string(rc.cam.n_dist) +
                            " coefficients is outside the camera models (0..2, at most 12 coefficients)";
            return FID_E_INVALID_ARG;
        }
        bool finite = true;
        for (int k = 0; k < 9; k++) finite = finite && rc.cam.K[k] - rc.cam.K[k] == 0 && rc.R[k] - rc.R[k] == 0;
        for (int k = 0; k < rc.cam.n_dist; k++) finite = finite && rc.cam.D[k] - rc.cam.D[k] == 0;
        for (int k = 0; k < 3; k++) finite = finite && rc.t[k] - rc.t[k] == 0;
        if (!finite) {
            c->last_error = who + "K, D, R and t must be finite";
            return FID_E_INVALID_ARG;
        }
        double worst = 0;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const double v = rc.R[a] * rc.R[b] + rc.R[3 + a] * rc.R[3 + b] + rc.R[6 + a] * rc.R[6 + b] - (a == b ? 1. : 0.);
                worst = fabs(v) > worst ? fabs(v) : worst;
            }
        const double det = rc.R[0] * (rc.R[4] * rc.R[8] - rc.R[5] * rc.R[7]) - rc.R[1] * (rc.R[3] * rc.R[8] - rc.R[5] * rc.R[6]) +
                           rc.R[2] * (rc.R[3] * rc.R[7] - rc.R[4] * rc.R[6]);
        if (worst > 1e-9 || det < 0) {
            c->last_error = who + "R is not a rotation (max |R^T R - I| = " + std::to_string(worst) + ", the bound is 1e-9; det R = " + std::to_string(det) + ")";
            return FID_E_INVALID_ARG;
        }
        tab[(size_t)i] = rc;
        tab[(size_t)i].cam = fid_camera_normalised(rc.cam);
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n == 0) {
        if (c->rig) c->rig->n = 0;
        return FID_OK;
    }
    if (!c->rig) {
        RigBufs *B = new (std::nothrow) RigBufs;
        if (!B) return FID_E_OUT_OF_MEMORY;
        const size_t slots = (size_t)c->lim.max_batch + 1;
        MemLayout l;
        l.add(&B->d_cams, FID_RIG_MAX_CAMERAS), l.add(&B->d_out, slots), l.add(&B->d_cov, slots), l.add(&B->d_cnt, FID_RIG_MAX_CAMERAS);
        hipError_t e = B->mem.reserve(l.bytes());
        if (e == hipSuccess) e = hipMemset(B->mem.p, 0, l.bytes());  // (no byte a caller is handed, padding included, is the allocator's)
        if (e != hipSuccess) delete B;
        HIPCHK(c, e);
        l.bind(B->mem.p);
        c->rig = B;  // (published when all of it exists)
    }
    // from here on the device table is being overwritten: a copy that fails leaves no rig rather than the old count beside a new table
    c->rig->n = 0;
    HIPCHK(c, hipMemcpy(c->rig->d_cams, tab.data(), sizeof(fid_rig_camera) * (size_t)n, hipMemcpyHostToDevice));
    c->rig->n = n;
    return FID_OK;
}

fid_status fid_rig_steps_last(fid_ctx *c, int32_t *n_steps)
{
    if (!c || !n_steps || c->last_frames <= 0) return FID_E_INVALID_ARG;
    if (!c->rig || c->rig->n == 0) {
        c->last_error = "no rig: fid_set_rig first";
        return FID_E_INVALID_ARG;
    }
    if (c->last_frames % c->rig->n != 0) {
        c->last_error = "the last call had " + std::to_string(c->last_frames) + " frames, no multiple of the rig's " + std::to_string(c->rig->n) + " cameras";
        return FID_E_INVALID_ARG;
    }
    *n_steps = c->last_frames / c->rig->n;
    return FID_OK;
}

static bool refuse_no_rig(fid_ctx *c)
{
    const bool none = !c->rig || c->rig->n == 0;
    if (none) c->last_error = "no rig: fid_set_rig first";
    return none;
}

// k_rig_pose for `steps` time steps on the context's stream, the records (and covariances) copied to the caller, synchronised
static fid_status rig_pose_run(fid_ctx *c, const fid_marker *d_markers, const int *d_n, int n_stride_ints, int per_frame, int steps, int slot0,
                               fid_rig_pose_out *out, double sigma_px, fid_map_pose_cov *cov)
{
    RigBufs *B = c->rig;
    fid_map_pose_cov *d_cov = cov ? B->d_cov + slot0 : nullptr;
    hipLaunchKernelGGL(k_rig_pose, dim3(steps), dim3(64), 0, c->stream, d_markers, d_n, n_stride_ints, per_frame, (const fid_rig_camera *)B->d_cams, B->n,
                       (const int *)c->d_map_ids, (const double *)c->d_map_obj, c->map_n, B->d_out + slot0, sigma_px, d_cov);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, B->d_out + slot0, sizeof(fid_rig_pose_out) * (size_t)steps, hipMemcpyDeviceToHost, c->stream));
    if (cov) HIPCHK(c, hipMemcpyAsync(cov, d_cov, sizeof(fid_map_pose_cov) * (size_t)steps, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FID_OK;
}

fid_status fid_rig_pose_last(fid_ctx *c, fid_rig_pose_out *out, int32_t cap_steps, double sigma_px, fid_map_pose_cov *cov)
{
    if (!c || !out || c->last_frames <= 0) return FID_E_INVALID_ARG;
    if (cov && !fid_sigma_usable(sigma_px)) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_map(c) || refuse_no_rig(c)) return FID_E_INVALID_ARG;
    const int C = c->rig->n, F = c->last_frames;
    if (F % C != 0) {
        c->last_error = "the last call had " + std::to_string(F) + " frames, no multiple of the rig's " + std::to_string(C) + " cameras";
        return FID_E_INVALID_ARG;
    }
    if (cap_steps < F / C) {
        c->last_error = "caller room for " + std::to_string(cap_steps) + " time steps, the last call had " + std::to_string(F / C);
        return FID_E_CAPACITY;
    }
    HIPCHK(c, hipSetDevice(c->device));
    return rig_pose_run(c, c->d_markers, &c->d_counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), c->P.maxMarkers, F / C, 0, out, sigma_px, cov);
}

fid_status fid_rig_pose(fid_ctx *c, const fid_marker *markers, const int32_t *n_per_camera, fid_rig_pose_out *out, double sigma_px, fid_map_pose_cov *cov)
{
    if (!c || !out || !n_per_camera) return FID_E_INVALID_ARG;
    if (cov && !fid_sigma_usable(sigma_px)) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_map(c) || refuse_no_rig(c)) return FID_E_INVALID_ARG;
    RigBufs *B = c->rig;
    long long total = 0;
    for (int i = 0; i < B->n; i++) {
        if (n_per_camera[i] < 0) return FID_E_INVALID_ARG;
        total += n_per_camera[i];
    }
    if (total > 0x3fffffff || (total > 0 && !markers)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int *d_total = nullptr;
    const fid_status rcs = stage_markers(c, B->in, markers, (int32_t)total, &d_total);
    if (rcs != FID_OK) return rcs;
    HIPCHK(c, hipMemcpyAsync(B->d_cnt, n_per_camera, sizeof(int) * (size_t)B->n, hipMemcpyHostToDevice, c->stream));
    return rig_pose_run(c, B->in.markers(), B->d_cnt, 1, 0, 1, c->lim.max_batch, out, sigma_px, cov);
}
