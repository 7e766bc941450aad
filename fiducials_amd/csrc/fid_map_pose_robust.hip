// fid_map_pose_robust.hip -- the map pose by consensus (fid_abi.h: "map pose that survives wrong markers").  Part of the fid_api.hip
// translation unit, behind fid_map_pose.hip, whose gather, tables (MpLds) and launch conventions it shares.
//
// ------------------------------------------------------------------------------------------------ K20: robust map pose
// One wave per frame (blockIdx.x: a batch is one launch):
//   (1) gather: k_map_pose's (mp_gather, mp_load_points), into the same LDS tables -- ALL used markers stay there; a solve reads a
//       subset through sub[].  mn is written after scoring (mp_store_mn): until then the counters of (3) lie there.
//   (2) eligibility (a ballot per 64 markers; uniform 4 x 64 bit masks in registers from here on) and the hypotheses: the rank of
//       every eligible marker by (area descending, k ascending), counted against the whole list; rank < 64 is a hypothesis and the
//       rank is its lane.
//   (3) scoring, lanes = hypotheses: every lane builds h_k (pnp_start_largest) and walks the eligible markers.  The lower median is
//       EXACT, by a radix select on the bit pattern of the (non-negative) double, 7 bits a pass: a pass recomputes the m errors and
//       counts those that carry the prefix chosen so far into 128 buckets (16 bit counters, [bucket][lane], 16 KB laid over the mn /
//       Mxy tables, which nothing needs yet); the bucket that holds rank (m - 1) / 2 extends the prefix.  A bucket with one member
//       ends the search one pass later (that pass remembers the member); otherwise nine passes spell all 63 bits.  Nothing is
//       rounded and nothing is stored per (lane, marker).
//   (4) the winner (smallest score bits, then lowest k: a butterfly), I_0 with lanes = markers, then up to four solves.  A solve is
//       fid_pnp.h's pnp_wave_solve, the one k_map_pose runs, over RbView: the subset's points in list order (point p of the subset
//       is point 4 sub[p / 4] + p % 4 of the tables, the largest marker is sought among the subset's): the same operands in the same
//       order of sums, so the record equals fid_map_pose_cam's on that subset.
// LDS: MpLds (63 760 B) + sub (256 B) + hyp (128 B).
struct RbLds {
    MpLds m;
    unsigned char sub[MP_MAX_USED];  // the subset being solved: used indices, ascending
    short hyp[64];                   // hypothesis of lane l: used index, or -1
};
static_assert(sizeof(RbLds) <= 64 * 1024, "k_map_pose_robust: static LDS");
static_assert(sizeof(unsigned short) * 128 * 64 <= sizeof(float) * MP_MAX_PTS * 4, "k_map_pose_robust: the counters lie over mn and Mxy");
static_assert(MP_MAX_USED <= 256, "k_map_pose_robust: sub[] holds bytes, the masks 4 x 64 bits");

// err(p, j): the largest distance over marker j's four corners between the image corner and the unrounded projection
template <int MODEL>
__device__ __forceinline__ double rb_err(const MpLds *s, int j, const double param[6], const double K[9], const double kd[12])
{
    double worst = 0.;
    for (int q = 0; q < 4; q++) {
        const int p = 4 * j + q;
        const double M[3] = {s->obj[p][0], s->obj[p][1], s->obj[p][2]};
        double Jrow[6];
        const double dx = project_one<MODEL>(M, param, K, kd, 0, Jrow, false) - s->img[p][0];
        const double dy = project_one<MODEL>(M, param, K, kd, 1, Jrow, false) - s->img[p][1];
        const double d = sqrt(dx * dx + dy * dy);
        if (!(d <= worst)) worst = d;  // (a NaN stays)
    }
    return worst;
}

__device__ __forceinline__ bool rb_bit(const unsigned long long m[4], int k) { return (m[k >> 6] >> (k & 63)) & 1ull; }

// fid_pnp.h's view of the subset sub[0..nsub): point i is point 4 sub[i / 4] + i % 4 of the tables, marker k is marker sub[k]; Mxy is
// written and read in subset order
struct RbView {
    RbLds *rs;
    int nsub;
    static constexpr bool PLANAR_ONLY = false;
    __device__ __forceinline__ int at(int i) const { return 4 * (int)rs->sub[i >> 2] + (i & 3); }
    __device__ __forceinline__ void obj(int i, double M[3]) const
    {
        const int q = at(i);
        for (int a = 0; a < 3; a++) M[a] = rs->m.obj[q][a];
    }
    __device__ __forceinline__ double img(int i, int c) const { return rs->m.img[at(i)][c]; }
    __device__ __forceinline__ float mn(int i, int c) const { return rs->m.mn[at(i)][c]; }
    __device__ __forceinline__ float *Mxy(int i) const { return rs->m.Mxy[i]; }
    __device__ __forceinline__ double *A() const { return rs->m.A; }
    __device__ __forceinline__ double *V() const { return rs->m.V; }
    __device__ __forceinline__ int markers() const { return nsub; }
    __device__ __forceinline__ double area(int k) const { return rs->m.area[rs->sub[k]]; }
    static constexpr bool MARKER_IN_PLACE = true;
    __device__ __forceinline__ PnpObj4 marker_obj(int k) const { return rs->m.obj + 4 * (int)rs->sub[k]; }
    __device__ __forceinline__ PnpImg4 marker_img(int k) const { return rs->m.img + 4 * (int)rs->sub[k]; }
};

// { j eligible : err(param, j) <= thr }, lanes = markers; every lane returns the same masks.  With stats: the largest err inside
// `in` and the smallest over the eligible markers outside it (-1 where there is none).
template <int MODEL, bool STATS>
__device__ __forceinline__ void rb_admit(const MpLds *s, int found, int lane, const unsigned long long elig[4], const double param[6], const double K[9],
                                         const double kd[12], double thr, unsigned long long set[4], const unsigned long long in[4], double *worst_in,
                                         double *best_out)
{
    double wi = -1., bo = -1.;
    for (int w = 0; w < 4; w++) {
        const int k = 64 * w + lane;
        bool ok = false;
        if (k < found && rb_bit(elig, k)) {
            const double e = rb_err<MODEL>(s, k, param, K, kd);
            ok = e <= thr;
            if constexpr (STATS) {
                if (rb_bit(in, k)) {
                    if (!(e <= wi)) wi = e;
                } else if (bo < 0. || e < bo) {
                    bo = e;
                }
            }
        }
        set[w] = __ballot(ok);
    }
    if constexpr (STATS) {
        for (int mask = 1; mask < 64; mask <<= 1) {
            const double wo = shfl_xor_f64(wi, mask), bb = shfl_xor_f64(bo, mask);
            if (!(wo <= wi)) wi = wo;
            if (bb >= 0. && (bo < 0. || bb < bo)) bo = bb;
        }
        *worst_in = wi;
        *best_out = bo;
    }
}

template <int MODEL>
__global__ __launch_bounds__(64) void k_map_pose_robust(const fid_marker *__restrict__ markers, const int *__restrict__ nmark_per_frame, int nmark_stride_ints,
                                                         int per_frame, const int *__restrict__ map_ids, const double *__restrict__ map_obj, int map_n,
                                                         PoseCam cam, double inlier_px, int min_markers, fid_map_pose_out *__restrict__ out,
                                                         fid_map_robust_out *__restrict__ rout)
{
    __shared__ RbLds rs;
    MpLds &s = rs.m;
    const int f = blockIdx.x, lane = threadIdx.x;
    const double *K = cam.K, *kd = cam.D;
    const fid_marker *mlist = markers + (long long)f * per_frame;
    // ---- (1) the frame's markers that the map names (k_map_pose's gather)
    int n_over;
    const int found = mp_gather(s, mlist, nmark_per_frame[(long long)f * nmark_stride_ints], per_frame, map_ids, map_n, lane, &n_over);
    // the record beside the pose: what every exit below starts from
    fid_map_robust_out ro;
    ro.status = FID_MAP_ROBUST_NO_MARKERS;
    ro.n_used = found;
    ro.n_inliers = 0;
    ro.n_outliers = found;
    ro.hypothesis = -1;
    ro.rounds = 0;
    ro.stable = 0;
    ro.reserved0 = 0;
    ro.score = ro.worst_inlier_px = ro.best_outlier_px = -1.;
    for (int i = 0; i < 4; i++) ro.outlier_mask[i] = 0ull;
    for (int i = 0; i < 16; i++) ro.outlier_index[i] = -1;
    if (found == 0) {
        if (lane == 0) {
            mp_pose_none(out + f, 0, 0, 0.);
            rout[f] = ro;
        }
        return;
    }
    SR_LDS_SYNC();
    const int npts = 4 * found;
    (void)mp_load_points<MODEL, false>(s, mlist, map_obj, found, lane, K, kd);
    SR_LDS_SYNC();
    // ---- (2) eligible markers (all four corners undistort) ...
    unsigned long long elig[4], I[4], Inext[4];
    int m_elig = 0;
    for (int w = 0; w < 4; w++) {
        const int k = 64 * w + lane;
        bool ok = k < found;
        if constexpr (MODEL == FID_CAM_EQUIDISTANT) {
            if (ok)
                for (int q = 0; q < 4; q++) {
                    double x, y;
                    ok = pnp_undistort<MODEL>(K, kd, s.img[4 * k + q][0], s.img[4 * k + q][1], &x, &y) && ok;
                }
        }
        elig[w] = __ballot(ok);
        m_elig += __builtin_popcountll(elig[w]);
    }
    // ... and the hypotheses: rank by (area descending, k ascending) among the eligible; rank < 64 takes lane `rank`
    rs.hyp[lane] = -1;
    SR_LDS_SYNC();
    for (int w = 0; w < 4; w++) {
        const int k = 64 * w + lane;
        if (k < found && rb_bit(elig, k)) {
            const double a = s.area[k];
            int rank = 0;
            for (int j = 0; j < found; j++)
                if (rb_bit(elig, j) && (s.area[j] > a || (s.area[j] == a && j < k))) rank++;
            if (rank < FID_MAP_ROBUST_HYPOTHESES) rs.hyp[rank] = (short)k;
        }
    }
    SR_LDS_SYNC();
    // ---- (3) score(k): the lower median of err(h_k, j) over the eligible j, exact (radix select on the bits, see the head of the file)
    const int hk = rs.hyp[lane];
    double hp[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long score_bits = ~0ull;
    if (hk >= 0) {
        const double *c0 = s.obj[4 * hk], *c2 = s.obj[4 * hk + 2];
        const double cc[3] = {0.5 * (c0[0] + c2[0]), 0.5 * (c0[1] + c2[1]), 0.5 * (c0[2] + c2[2])};
        pnp_start_largest<MODEL>(c0, s.obj[4 * hk + 1], s.obj[4 * hk + 3], cc, s.img + 4 * hk, K, kd, hp);
        unsigned short *cnt = (unsigned short *)&s.mn[0][0] + lane;  // counter of bucket b: cnt[64 * b]
        unsigned long long prefix = 0ull;
        int rank = (m_elig - 1) / 2, members = m_elig;
        for (int shift = 56; shift >= 0; shift -= 7) {
            for (int b = 0; b < 128; b++) cnt[64 * b] = 0;
            unsigned long long last = 0ull;
            for (int j = 0; j < found; j++) {
                if (!rb_bit(elig, j)) continue;
                const unsigned long long bits = (unsigned long long)__double_as_longlong(rb_err<MODEL>(&s, j, hp, K, kd)) & 0x7fffffffffffffffull;
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
    SR_LDS_SYNC();  // (the counters lay over mn and Mxy)
    // the undistorted image points as floats (the DLT's input), for every used point: a solve reads its subset's
    for (int p = lane; p < npts; p += 64) (void)mp_store_mn<MODEL>(s, p, s.img[p][0], s.img[p][1], K, kd);
    // ---- (4) the winner: the smallest score, then the lowest k
    int win_k = hk >= 0 ? hk : 0x7fffffff, win_lane = lane;
    unsigned long long win_bits = score_bits;
    for (int mask = 1; mask < 64; mask <<= 1) {
        const unsigned lo = __shfl_xor((unsigned)win_bits, mask, WAVE), hi = __shfl_xor((unsigned)(win_bits >> 32), mask, WAVE);
        const unsigned long long ob = ((unsigned long long)hi << 32) | lo;
        const int ok = __shfl_xor(win_k, mask, WAVE), ol = __shfl_xor(win_lane, mask, WAVE);
        if (ob < win_bits || (ob == win_bits && ok < win_k)) {
            win_bits = ob;
            win_k = ok;
            win_lane = ol;
        }
    }
    double param[6], image_error = 0.;
    int nI = 0, rounds = 0, stable = 0, status = FID_MAP_ROBUST_NO_CONSENSUS;
    for (int w = 0; w < 4; w++) I[w] = 0ull;
    if (m_elig > 0) {
        for (int i = 0; i < 6; i++) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(hp[i]);
            const unsigned lo = __shfl((unsigned)u, win_lane, WAVE), hi = __shfl((unsigned)(u >> 32), win_lane, WAVE);
            param[i] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
        const double score = __longlong_as_double((long long)win_bits);
        ro.hypothesis = s.mk[win_k];
        ro.score = score;
        const double thr0 = fmax(inlier_px, 3. * score);
        rb_admit<MODEL, false>(&s, found, lane, elig, param, K, kd, thr0, I, I, nullptr, nullptr);
        for (int w = 0; w < 4; w++) nI += __builtin_popcountll(I[w]);
        // ---- the rounds
        while (nI >= min_markers && nI > 0) {
            // the subset in list order
            int before = 0;
            for (int w = 0; w < 4; w++) {
                const int k = 64 * w + lane;
                if ((I[w] >> lane) & 1ull) rs.sub[before + __builtin_popcountll(I[w] & ((1ull << lane) - 1ull))] = (unsigned char)k;
                before += __builtin_popcountll(I[w]);
            }
            SR_LDS_SYNC();
            pnp_wave_solve<MODEL>(RbView{&rs, nI}, 4 * nI, lane, K, kd, param, &image_error);
            rounds++;
            double wi, bo;
            rb_admit<MODEL, true>(&s, found, lane, elig, param, K, kd, inlier_px, Inext, I, &wi, &bo);
            ro.worst_inlier_px = wi;
            ro.best_outlier_px = bo;
            int nnext = 0;
            for (int w = 0; w < 4; w++) nnext += __builtin_popcountll(Inext[w]);
            if (Inext[0] == I[0] && Inext[1] == I[1] && Inext[2] == I[2] && Inext[3] == I[3]) {
                stable = 1;
                status = FID_MAP_ROBUST_OK;
                break;
            }
            if (nnext < min_markers) {
                nI = 0;  // (no consensus: the pose solved is not returned)
                break;
            }
            if (rounds == FID_MAP_ROBUST_SOLVES) {
                status = FID_MAP_ROBUST_OK;
                break;
            }
            SR_LDS_SYNC();  // (sub[] is rewritten)
            for (int w = 0; w < 4; w++) I[w] = Inext[w];
            nI = nnext;
        }
    }
    if (lane == 0) {
        fid_map_pose_out o;
        ro.status = status;
        ro.rounds = rounds;
        ro.stable = stable;
        if (status == FID_MAP_ROBUST_OK) {
            o.n_markers = nI;
            o.n_over = n_over;
            pnp_pose_record(o, param, image_error);
            ro.n_inliers = nI;
            ro.n_outliers = found - nI;
            int no = 0;
            for (int k = 0; k < found; k++)
                if (!rb_bit(I, k)) {
                    ro.outlier_mask[k >> 6] |= 1ull << (k & 63);
                    if (no < 16) ro.outlier_index[no] = s.mk[k];
                    no++;
                }
        } else {
            o.n_markers = 0;
            o.n_over = 0;
            pnp_pose_record_zero(o, 0.);
            ro.worst_inlier_px = ro.best_outlier_px = -1.;
            int no = 0;
            for (int k = 0; k < found; k++) {
                ro.outlier_mask[k >> 6] |= 1ull << (k & 63);
                if (no < 16) ro.outlier_index[no] = s.mk[k];
                no++;
            }
        }
        out[f] = o;
        rout[f] = ro;
    }
}

// the kernel for F frames on stream st
static void map_pose_robust_launch(fid_ctx *c, hipStream_t st, const fid_marker *d_markers, const int *d_n, int n_stride_ints, int per_frame, int F,
                                   const fid_camera &camera, const fid_map_robust_opts &opts, fid_map_pose_out *d_out, fid_map_robust_out *d_rout)
{
    const PoseCam cam = pose_cam_from(camera, 0.);
    POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_map_pose_robust<CAM_MODEL>, dim3(F), dim3(64), 0, st, d_markers, d_n, n_stride_ints, per_frame,
                                                    (const int *)c->d_map_ids, (const double *)c->d_map_obj, c->map_n, cam, opts.inlier_px,
                                                    (int)opts.min_markers, d_out, d_rout));
}

static inline bool fid_robust_opts_usable(const fid_map_robust_opts *o)
{
    return o && o->inlier_px > 0. && o->inlier_px - o->inlier_px == 0. && o->min_markers >= 1;
}

// max_batch + 1 pose records and robust records of the robust call's own (the first robust call allocates them): d_mposes keeps
// what fid_map_pose_last* put there
static fid_status ensure_map_robust(fid_ctx *c)
{
    if (c->d_mrob) return FID_OK;
    const size_t n = (size_t)(c->lim.max_batch + 1);
    MemLayout dl, hl;
    dl.add(&c->d_rposes, n), dl.add(&c->d_mrob, n);
    hl.add(&c->h_rposes, n), hl.add(&c->h_mrob, n);
    return alloc_bound(c, c->rob_mem, dl, c->rob_hmem, hl);
}

fid_status fid_map_pose_robust_last_cam(fid_ctx *c, const fid_camera *camera, const fid_map_robust_opts *opts, fid_map_pose_out *pose_out,
                                        fid_map_robust_out *robust_out, int32_t cap_frames)
{
    if (!c || !fid_camera_usable(camera) || !pose_out || !robust_out || !fid_robust_opts_usable(opts) || c->last_frames <= 0) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_map(c)) return FID_E_INVALID_ARG;
    if (refuse_room(c, cap_frames)) return FID_E_CAPACITY;
    const int F = c->last_frames;
    HIPCHK(c, hipSetDevice(c->device));
    const fid_status rca = ensure_map_robust(c);
    if (rca != FID_OK) return rca;
    const PoseAsk ask = {fid_camera_normalised(*camera), 0., false, 0., {opts->inlier_px, opts->min_markers, 0}};
    if (!c->rob_req.answers(ask)) {
        map_pose_robust_launch(c, c->stream, c->d_markers, &c->d_counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), c->P.maxMarkers, F, ask.cam,
                               ask.opts, c->d_rposes, c->d_mrob);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_rposes, c->d_rposes, sizeof(fid_map_pose_out) * (size_t)F, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_mrob, c->d_mrob, sizeof(fid_map_robust_out) * (size_t)F, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->rob_req.answered(ask);
    }
    memcpy(pose_out, c->h_rposes, sizeof(fid_map_pose_out) * (size_t)F);
    memcpy(robust_out, c->h_mrob, sizeof(fid_map_robust_out) * (size_t)F);
    return FID_OK;
}

fid_status fid_map_pose_robust_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, int32_t n, const fid_map_robust_opts *opts,
                                   fid_map_pose_out *pose_out, fid_map_robust_out *robust_out)
{
    if (!c || !fid_camera_usable(camera) || !pose_out || !robust_out || !fid_robust_opts_usable(opts) || n < 0 || (n > 0 && !markers))
        return FID_E_INVALID_ARG;
    if (refuse_in_flight(c) || refuse_no_map(c)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int *d_n = nullptr;
    fid_status rca = stage_markers(c, c->map_in, markers, n, &d_n);
    if (rca == FID_OK) rca = ensure_map_robust(c);
    if (rca != FID_OK) return rca;
    fid_map_pose_out *d_out = c->d_rposes + c->lim.max_batch;  // (the slot behind a batch's: the last call's results stay)
    fid_map_robust_out *d_rout = c->d_mrob + c->lim.max_batch;
    map_pose_robust_launch(c, c->stream, c->map_in.markers(), d_n, 0, n > 0 ? n : 1, 1, *camera, *opts, d_out, d_rout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(pose_out, d_out, sizeof(fid_map_pose_out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(robust_out, d_rout, sizeof(fid_map_robust_out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FID_OK;
}
