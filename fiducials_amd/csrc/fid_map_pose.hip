// fid_map_pose.hip -- one camera pose per frame from a map of fiducials (fid_abi.h).  Part of the fid_api.hip translation unit,
// behind fid_stag.hip.  The solve itself -- planarity, the start, CvLevMarq, the reprojection error -- is fid_pnp.h's wave-strided
// pnp_wave_solve, which k_map_pose_robust and k_charuco_pose run as well; this file gathers the points it runs on.
//
// ------------------------------------------------------------------------------------------------ K19: map pose
// cv::aruco::estimatePoseBoard: cv::solvePnP (ITERATIVE) over the four corners of every marker of a frame that the map names.
// One wave per frame (blockIdx.x: a batch is one launch):
//   (1) gather (mp_gather, shared with k_map_pose_robust).  Lanes take the markers of the frame's list 64 at a time and binary-search
//       the id in the map's sorted id table.  A first pass marks every map entry that is hit (a bit per entry in LDS, set with an
//       atomic or; a second hit sets the entry's bit in a second table): an id that occurs more than once in the frame is left out
//       altogether.  The second pass compacts the survivors in list order (ballot + prefix count) and stops filling at MP_MAX_USED;
//       the rest are counted.  Then the points (mp_load_points): object points (the map's, double) and image points (the float
//       corners widened) go to LDS, with the undistorted image point rounded to float (findHomography's input) and the marker's
//       image area.
//   (2)-(4) pnp_wave_solve over MpView, the tables as they stand: planarity, the DLT start of a coplanar set or the largest marker's
//       closed-form pose, CvLevMarq with the camera model's distortion (the template parameter), the reprojection error.  Point p is
//       on lane p % 64; every sum is per-lane partial sums in point order followed by one xor butterfly: a fixed order, reproducible
//       from run to run, the same value in every lane.
// LDS: 24 KB object points + 16 KB image points (the 40 KB of 1 024 points) + 16 KB of float pairs for the DLT + 7 KB of tables.
#include <algorithm>

#define MP_MAX_USED FID_MAP_MAX_USED
#define MP_MAX_PTS (4 * MP_MAX_USED)
#define MP_BIT_WORDS (FID_MAP_MAX_ENTRIES / 32)
struct MpLds {
    double obj[MP_MAX_PTS][3], img[MP_MAX_PTS][2];
    float mn[MP_MAX_PTS][2], Mxy[MP_MAX_PTS][2];
    double A[81], V[81], area[MP_MAX_USED];
    int mk[MP_MAX_USED], ent[MP_MAX_USED];
    unsigned seen[MP_BIT_WORDS], dup[MP_BIT_WORDS];
};
static_assert(sizeof(MpLds) <= 64 * 1024, "k_map_pose: static LDS");

// index of id in the ascending table ids[0..n), or -1
__device__ __forceinline__ int mp_find(const int *__restrict__ ids, int n, int id)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < n && ids[lo] == id) ? lo : -1;
}

// stage (1) of k_map_pose and k_map_pose_robust: the frame's markers that the map names, in list order, without the ids seen twice,
// as s.mk (index in the list) and s.ent (entry of the map).  Returns how many are used (at most MP_MAX_USED), *n_over: those beyond.
__device__ __forceinline__ int mp_gather(MpLds &s, const fid_marker *__restrict__ mlist, int nm, int per_frame, const int *__restrict__ map_ids, int map_n,
                                         int lane, int *n_over)
{
    nm = nm < 0 ? 0 : (nm > per_frame ? per_frame : nm);
    map_n = map_n > FID_MAP_MAX_ENTRIES ? FID_MAP_MAX_ENTRIES : map_n;
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
    *n_over = found > MP_MAX_USED ? found - MP_MAX_USED : 0;
    return found - *n_over;
}

// the undistorted image point of point p rounded to float (the DLT's input: findHomography converts to float); false: (u, v) lies
// beyond the (equidistant) model
template <int MODEL>
__device__ __forceinline__ bool mp_store_mn(MpLds &s, int p, double u, double v, const double K[9], const double kd[12])
{
    double x, y;
    const bool ok = pnp_undistort<MODEL>(K, kd, u, v, &x, &y);
    s.mn[p][0] = (float)x;
    s.mn[p][1] = (float)y;
    return ok;
}

// the points of the found markers: object points (the map's, double), image points (the float corners widened), the marker's image
// area and, with MN, mn in the same pass (k_map_pose_robust writes mn later, its counters lie there until scoring is done; a
// pass of its own behind this one measured slower for k_map_pose).  False in a lane that met a corner beyond the model.
template <int MODEL, bool MN>
__device__ __forceinline__ bool mp_load_points(MpLds &s, const fid_marker *__restrict__ mlist, const double *__restrict__ map_obj, int found, int lane,
                                               const double K[9], const double kd[12])
{
    bool posable = true;
    for (int p = lane; p < 4 * found; p += 64) {
        const int k = p >> 2, q = p & 3;
        const fid_marker *mk = mlist + s.mk[k];
        const double *src = map_obj + (size_t)s.ent[k] * 12 + q * 3;
        for (int a = 0; a < 3; a++) s.obj[p][a] = src[a];
        const double u = (double)mk->corners[2 * q], v = (double)mk->corners[2 * q + 1];
        s.img[p][0] = u;
        s.img[p][1] = v;
        if constexpr (MN) {
            const bool ok = mp_store_mn<MODEL>(s, p, u, v, K, kd);
            if constexpr (MODEL == FID_CAM_EQUIDISTANT) posable = posable && ok;
        }
        if (q == 0) {  // the marker's area in the image (shoelace over its four corners)
            double a2 = 0;
            for (int i = 0; i < 4; i++) {
                const int i1 = (i + 1) & 3;
                a2 += (double)mk->corners[2 * i] * (double)mk->corners[2 * i1 + 1] - (double)mk->corners[2 * i1] * (double)mk->corners[2 * i + 1];
            }
            s.area[k] = fabs(a2);
        }
    }
    return posable;
}

// fid_pnp.h's view of all found markers' points: the tables as they stand
struct MpView {
    MpLds *s;
    int found;
    static constexpr bool PLANAR_ONLY = false;
    __device__ __forceinline__ void obj(int i, double M[3]) const
    {
        for (int a = 0; a < 3; a++) M[a] = s->obj[i][a];
    }
    __device__ __forceinline__ double img(int i, int c) const { return s->img[i][c]; }
    __device__ __forceinline__ float mn(int i, int c) const { return s->mn[i][c]; }
    __device__ __forceinline__ float *Mxy(int i) const { return s->Mxy[i]; }
    __device__ __forceinline__ double *A() const { return s->A; }
    __device__ __forceinline__ double *V() const { return s->V; }
    __device__ __forceinline__ int markers() const { return found; }
    __device__ __forceinline__ double area(int k) const { return s->area[k]; }
    static constexpr bool MARKER_IN_PLACE = false;
    __device__ __forceinline__ int first(int k) const { return 4 * k; }
};

// a frame's record without a pose (no marker of the map; a corner beyond the model)
__device__ __forceinline__ void mp_pose_none(fid_map_pose_out *dst, int n_markers, int n_over, double image_error)
{
    fid_map_pose_out o;
    o.n_markers = n_markers;
    o.n_over = n_over;
    pnp_pose_record_zero(o, image_error);
    *dst = o;
}

// COV: the covariance tail (fid_abi.h: "pose covariance") over the same points -- the selection above it is this one body's --: J^T J
// from pnp_wave_residuals, the sums of the Levenberg-Marquardt loop without J^T e; it also writes cov_cam_pose.  The COV = true form
// takes (double sigma_px, fid_map_pose_cov *cov) as the pack CovArgs, so that the COV = false form has the parameter list it always
// had AND stays the kernel's own body: moved into an _impl function behind two __global__ wrappers (the STag kernels' form, which
// they had before) the COV = false kernel came out scheduled and allocated differently.  What the body shares is below it, not
// around it: the gather, the point load, the solve and the record are calls into inlined functions.  k_map_pose_cov<MODEL> names the
// COV = true instantiation.
struct MapPoseCovArgs {
    double sigma_px;
    fid_map_pose_cov *cov;
};
template <int MODEL, bool COV = false, class... CovArgs>
__global__ __launch_bounds__(64) void k_map_pose(const fid_marker *__restrict__ markers, const int *__restrict__ nmark_per_frame, int nmark_stride_ints,
                                                  int per_frame, const int *__restrict__ map_ids, const double *__restrict__ map_obj, int map_n,
                                                  PoseCam cam, fid_map_pose_out *__restrict__ out, CovArgs... cov_args)
{
    static_assert(sizeof...(CovArgs) == (COV ? 2 : 0), "k_map_pose: (sigma_px, cov) with COV, nothing without");
    __shared__ MpLds s;
    const int f = blockIdx.x, lane = threadIdx.x;
    const double *K = cam.K, *kd = cam.D;
    const fid_marker *mlist = markers + (long long)f * per_frame;
    // ---- (1) the frame's markers that the map names
    int n_over;
    const int found = mp_gather(s, mlist, nmark_per_frame[(long long)f * nmark_stride_ints], per_frame, map_ids, map_n, lane, &n_over);
    if (found == 0) {
        if (lane == 0) {
            mp_pose_none(out + f, 0, 0, 0.);
            if constexpr (COV) {
                fid_map_pose_cov *cov = MapPoseCovArgs{cov_args...}.cov;
                pnp_cov_zero(&cov[f].pose, 1, 0, cov[f].cov_cam_pose);
            }
        }
        return;
    }
    SR_LDS_SYNC();
    const int npts = 4 * found;
    const bool posable = mp_load_points<MODEL, true>(s, mlist, map_obj, found, lane, K, kd);
    SR_LDS_SYNC();
    if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
        if (__ballot(!posable) != 0ull) {  // a corner beyond the model (fid_abi.h: "a marker that cannot be posed") voids the frame's record
            if (lane == 0) {
                mp_pose_none(out + f, found, n_over, -1.);
                if constexpr (COV) {
                    fid_map_pose_cov *cov = MapPoseCovArgs{cov_args...}.cov;
                    pnp_cov_zero(&cov[f].pose, 1, npts, cov[f].cov_cam_pose);
                }
            }
            return;
        }
    }
    // ---- (2)-(4) and the reprojection error over all of them
    const MpView view = {&s, found};
    double param[6], image_error;
    pnp_wave_solve<MODEL>(view, npts, lane, K, kd, param, &image_error);
    if (lane == 0) {
        fid_map_pose_out o;
        o.n_markers = found;
        o.n_over = n_over;
        pnp_pose_record(o, param, image_error);
        out[f] = o;
    }
    if constexpr (COV) {
        // ---- the covariance: J and e at the returned param, summed as the Levenberg-Marquardt sums are
        double S[21];
        const double e2 = wave_sum_f64(pnp_wave_residuals<MODEL, false>(view, npts, lane, K, kd, param, true, S, nullptr));
        const MapPoseCovArgs ca = {cov_args...};
        if (lane == 0) pnp_covariance<true>(S, e2, npts, param, ca.sigma_px, &ca.cov[f].pose, ca.cov[f].cov_cam_pose);
    }
}
template <int MODEL>
constexpr auto k_map_pose_cov = k_map_pose<MODEL, true, double, fid_map_pose_cov *>;

// the kernel for F frames on stream st (fid_api.hip's enqueue_detect calls it for the batch it has just enqueued)
static void map_pose_launch(fid_ctx *c, hipStream_t st, const fid_marker *d_markers, const int *d_n, int n_stride_ints, int per_frame, int F,
                            const fid_camera &camera, fid_map_pose_out *d_out, bool with_cov, double sigma_px, fid_map_pose_cov *d_cov)
{
    const PoseCam cam = pose_cam_from(camera, 0.);
    if (with_cov) {
        POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_map_pose_cov<CAM_MODEL>, dim3(F), dim3(64), 0, st, d_markers, d_n, n_stride_ints, per_frame,
                                                        (const int *)c->d_map_ids, (const double *)c->d_map_obj, c->map_n, cam, d_out, sigma_px, d_cov));
        return;
    }
    POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_map_pose<CAM_MODEL>, dim3(F), dim3(64), 0, st, d_markers, d_n, n_stride_ints, per_frame,
                                                    (const int *)c->d_map_ids, (const double *)c->d_map_obj, c->map_n, cam, d_out));
}

fid_status fid_set_map(fid_ctx *c, const fid_map_entry *entries, int32_t n)
{
    if (!c || n < 0 || (n > 0 && !entries) || refuse_in_flight(c)) return FID_E_INVALID_ARG;
    if (n > FID_MAP_MAX_ENTRIES) {
        c->last_error = "a map holds at most " + std::to_string(FID_MAP_MAX_ENTRIES) + " entries (FID_MAP_MAX_ENTRIES), not " + std::to_string(n);
        return FID_E_UNSUPPORTED;
    }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) {
        order[(size_t)i] = i;
        const fid_map_entry &e = entries[i];
        bool finite = e.len - e.len == 0;
        for (int k = 0; k < 9; k++) finite = finite && e.R[k] - e.R[k] == 0;
        for (int k = 0; k < 3; k++) finite = finite && e.t[k] - e.t[k] == 0;
        if (!(e.len > 0) || !finite) {
            c->last_error = "map entry " + std::to_string(i) + " (id " + std::to_string(e.id) + "): len must be positive and the transform finite";
            return FID_E_INVALID_ARG;
        }
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return entries[a].id < entries[b].id; });
    for (int i = 1; i < n; i++)
        if (entries[order[(size_t)i]].id == entries[order[(size_t)i - 1]].id) {
            c->last_error = "map: id " + std::to_string(entries[order[(size_t)i]].id) + " is listed twice";
            return FID_E_INVALID_ARG;
        }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->map_req.forget();  // (the poses at hand are the old map's)
    c->rob_req.forget();
    if (n == 0) {
        c->map_n = 0;
        return FID_OK;
    }
    if (!c->d_map_ids) {
        // the first map of this context: the tables at their largest, a result slot per frame of a batch (device and pinned host)
        MemLayout dl, hl;
        dl.add(&c->d_map_ids, FID_MAP_MAX_ENTRIES), dl.add(&c->d_map_obj, 12 * FID_MAP_MAX_ENTRIES), dl.add(&c->d_mposes, (size_t)(c->lim.max_batch + 1));
        hl.add(&c->h_mposes, (size_t)(c->lim.max_batch + 1));
        const fid_status rca = alloc_bound(c, c->map_mem, dl, c->map_hmem, hl);
        if (rca != FID_OK) return rca;
    }
    std::vector<int> ids((size_t)n);
    std::vector<double> obj((size_t)n * 12);
    for (int i = 0; i < n; i++) {
        const fid_map_entry &e = entries[order[(size_t)i]];
        ids[(size_t)i] = e.id;
        const double h = (double)(float)(e.len / 2);  // (getSingleMarkerObjectPoints: Point3f)
        const double cx[4] = {-h, h, h, -h}, cy[4] = {h, h, -h, -h};
        for (int q = 0; q < 4; q++)
            for (int a = 0; a < 3; a++) obj[(size_t)i * 12 + q * 3 + a] = e.R[3 * a] * cx[q] + e.R[3 * a + 1] * cy[q] + e.t[a];
    }
    HIPCHK(c, hipMemcpy(c->d_map_ids, ids.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_map_obj, obj.data(), sizeof(double) * 12 * (size_t)n, hipMemcpyHostToDevice));
    c->map_n = n;
    return FID_OK;
}

fid_status fid_map_pose_last(fid_ctx *c, const double K[9], const double D[5], fid_map_pose_out *out, int32_t cap_frames)
{
    if (!K) return FID_E_INVALID_ARG;
    const fid_camera cam = fid_camera_plumb_bob(K, D);
    return fid_map_pose_last_cam(c, &cam, out, cap_frames);
}

// max_batch + 1 fid_map_pose_cov beside d_mposes / h_mposes (the first _cov call allocates them)
static fid_status ensure_map_cov(fid_ctx *c)
{
    if (c->d_mcov) return FID_OK;
    MemLayout dl, hl;
    dl.add(&c->d_mcov, (size_t)(c->lim.max_batch + 1));
    hl.add(&c->h_mcov, (size_t)(c->lim.max_batch + 1));
    return alloc_bound(c, c->mcov_mem, dl, c->mcov_hmem, hl);
}

// fid_map_pose_last_cam and fid_map_pose_last_cov_cam: the camera pose (with_cov: and its covariance) of every frame of the last call
static fid_status map_pose_last_run(fid_ctx *c, const fid_camera *camera, fid_map_pose_out *out, int32_t cap_frames, bool with_cov, double sigma_px,
                                    fid_map_pose_cov *cov)
{
    if (!c || !fid_camera_usable(camera) || !out || c->last_frames <= 0) return FID_E_INVALID_ARG;
    if (with_cov && (!cov || !fid_sigma_usable(sigma_px))) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_map(c)) return FID_E_INVALID_ARG;
    if (refuse_room(c, cap_frames)) return FID_E_CAPACITY;
    const int F = c->last_frames;
    HIPCHK(c, hipSetDevice(c->device));
    if (with_cov) {
        const fid_status rca = ensure_map_cov(c);
        if (rca != FID_OK) return rca;
    }
    const PoseAsk ask = {fid_camera_normalised(*camera), 0., with_cov, sigma_px, {}};
    if (!c->map_req.answers(ask)) {  // (else the detect call already ran k_map_pose, or its COV form, for this camera on these markers)
        map_pose_launch(c, c->stream, c->d_markers, &c->d_counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), c->P.maxMarkers, F, ask.cam, c->d_mposes,
                        with_cov, sigma_px, c->d_mcov);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_mposes, c->d_mposes, sizeof(fid_map_pose_out) * (size_t)F, hipMemcpyDeviceToHost, c->stream));
        if (with_cov) HIPCHK(c, hipMemcpyAsync(c->h_mcov, c->d_mcov, sizeof(fid_map_pose_cov) * (size_t)F, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->map_req.answered(ask);  // (asked for without its covariance: the next call runs k_map_pose's COV = false form)
    }
    memcpy(out, c->h_mposes, sizeof(fid_map_pose_out) * (size_t)F);
    if (with_cov) memcpy(cov, c->h_mcov, sizeof(fid_map_pose_cov) * (size_t)F);
    return FID_OK;
}

fid_status fid_map_pose_last_cam(fid_ctx *c, const fid_camera *camera, fid_map_pose_out *out, int32_t cap_frames)
{
    return map_pose_last_run(c, camera, out, cap_frames, false, 0., nullptr);
}

fid_status fid_map_pose_last_cov_cam(fid_ctx *c, const fid_camera *camera, fid_map_pose_out *out, int32_t cap_frames, double sigma_px,
                                     fid_map_pose_cov *cov)
{
    return map_pose_last_run(c, camera, out, cap_frames, true, sigma_px, cov);
}

fid_status fid_map_pose(fid_ctx *c, const double K[9], const double D[5], const fid_marker *markers, int32_t n, fid_map_pose_out *out)
{
    if (!K) return FID_E_INVALID_ARG;
    const fid_camera cam = fid_camera_plumb_bob(K, D);
    return fid_map_pose_cam(c, &cam, markers, n, out);
}

static fid_status map_pose_cam_run(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, int32_t n, fid_map_pose_out *out, bool with_cov,
                                   double sigma_px, fid_map_pose_cov *cov)
{
    if (!c || !fid_camera_usable(camera) || !out || n < 0 || (n > 0 && !markers)) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_map(c)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int *d_n = nullptr;
    const fid_status rcs = stage_markers(c, c->map_in, markers, n, &d_n);
    if (rcs != FID_OK) return rcs;
    fid_map_pose_out *d_out = c->d_mposes + c->lim.max_batch;  // (the slot behind a batch's: the last call's results stay)
    if (with_cov) {
        const fid_status rca = ensure_map_cov(c);
        if (rca != FID_OK) return rca;
    }
    fid_map_pose_cov *d_cov = with_cov ? c->d_mcov + c->lim.max_batch : nullptr;
    map_pose_launch(c, c->stream, c->map_in.markers(), d_n, 0, n > 0 ? n : 1, 1, *camera, d_out, with_cov, sigma_px, d_cov);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, sizeof(fid_map_pose_out), hipMemcpyDeviceToHost, c->stream));
    if (with_cov) HIPCHK(c, hipMemcpyAsync(cov, d_cov, sizeof(fid_map_pose_cov), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FID_OK;
}

fid_status fid_map_pose_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, int32_t n, fid_map_pose_out *out)
{
    return map_pose_cam_run(c, camera, markers, n, out, false, 0., nullptr);
}

fid_status fid_map_pose_cov_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, int32_t n, fid_map_pose_out *out, double sigma_px,
                                fid_map_pose_cov *cov)
{
    if (!cov || !fid_sigma_usable(sigma_px)) return FID_E_INVALID_ARG;
    return map_pose_cam_run(c, camera, markers, n, out, true, sigma_px, cov);
}
