// fid_map_pose_robust.hip -- the map pose by consensus (fid_abi.h: "map pose that survives wrong markers").  Part of the fid_api.hip
// translation unit, behind fid_map_pose.hip, whose gather, tables (MpLds) and launch conventions it shares.
//
// ------------------------------------------------------------------------------------------------ K20: robust map pose
// One wave per frame (blockIdx.x: a batch is one launch):
//   (1) gather: k_map_pose's own, into the same LDS tables -- ALL used markers stay there; a solve reads a subset through sub[].
//   (2) eligibility (a ballot per 64 markers; uniform 4 x 64 bit masks in registers from here on) and the hypotheses: the rank of
//       every eligible marker by (area descending, k ascending), counted against the whole list; rank < 64 is a hypothesis and the
//       rank is its lane.
//   (3) scoring, lanes = hypotheses: every lane builds h_k (pnp_start_largest) and walks the eligible markers.  The lower median is
//       EXACT, by a radix select on the bit pattern of the (non-negative) double, 7 bits a pass: a pass recomputes the m errors and
//       counts those that carry the prefix chosen so far into 128 buckets (16 bit counters, [bucket][lane], 16 KB laid over the mn /
//       Mxy tables, which nothing needs yet); the bucket that holds rank (m - 1) / 2 extends the prefix.  A bucket with one member
//       ends the search one pass later (that pass remembers the member); otherwise nine passes spell all 63 bits.  Nothing is
//       rounded and nothing is stored per (lane, marker).
//   (4) the winner (smallest score bits, then lowest k: a butterfly), I_0 with lanes = markers, then up to four solves.  rb_solve is
//       stages (2)-(4) of k_map_pose and its reprojection error, statement for statement, over the subset's points in list order
//       (point p of the subset is point 4 sub[p / 4] + p % 4 of the tables): the same operands in the same order of sums, so the
//       record equals fid_map_pose_cam's on that subset.  k_map_pose keeps its own body (see its comment on scheduling).
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

// mp_homography_dlt over the subset: correspondence i is Mxy[i] (written in subset order) -> mn[4 sub[i / 4] + i % 4]
__device__ bool rb_homography_dlt(RbLds *rs, int n, int lane, double H[9])
{
    MpLds *s = &rs->m;
#define RB_Q(i) (4 * (int)rs->sub[(i) >> 2] + ((i) & 3))
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    for (int i = lane; i < n; i += 64) {
        const int q = RB_Q(i);
        cmx += s->mn[q][0];
        cmy += s->mn[q][1];
        cMx += s->Mxy[i][0];
        cMy += s->Mxy[i][1];
    }
    cmx = wave_sum_f64(cmx) / n; cmy = wave_sum_f64(cmy) / n; cMx = wave_sum_f64(cMx) / n; cMy = wave_sum_f64(cMy) / n;
    for (int i = lane; i < n; i += 64) {
        const int q = RB_Q(i);
        smx += fabs(s->mn[q][0] - cmx);
        smy += fabs(s->mn[q][1] - cmy);
        sMx += fabs(s->Mxy[i][0] - cMx);
        sMy += fabs(s->Mxy[i][1] - cMy);
    }
    smx = wave_sum_f64(smx); smy = wave_sum_f64(smy); sMx = wave_sum_f64(sMx); sMy = wave_sum_f64(sMy);
    if (!(fabs(smx) >= DBL_EPSILON) || !(fabs(smy) >= DBL_EPSILON) || !(fabs(sMx) >= DBL_EPSILON) || !(fabs(sMy) >= DBL_EPSILON)) return false;
    smx = n / smx; smy = n / smy; sMx = n / sMx; sMy = n / sMy;
    for (int j = 0; j < 9; j++)
        for (int k = j; k < 9; k++) {
            double acc = 0;
            for (int i = lane; i < n; i += 64) {
                const int q = RB_Q(i);
                const double x = (s->mn[q][0] - cmx) * smx, y = (s->mn[q][1] - cmy) * smy;
                const double X = (s->Mxy[i][0] - cMx) * sMx, Y = (s->Mxy[i][1] - cMy) * sMy;
                double lxj, lyj, lxk, lyk;
                pnp_dlt_entry(j, X, Y, x, y, &lxj, &lyj);
                pnp_dlt_entry(k, X, Y, x, y, &lxk, &lyk);
                acc += lxj * lxk + lyj * lyk;
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) {
                s->A[j * 9 + k] = acc;
                s->A[k * 9 + j] = acc;
            }
        }
    return pnp_dlt_finish(s->A, s->V, lane, cmx, cmy, smx, smy, cMx, cMy, sMx, sMy, H);
}

// stages (2)-(4) of k_map_pose over the nsub markers sub[0..nsub) and getReprojectionError over them; every lane returns the same
template <int MODEL>
__device__ void rb_solve(RbLds *rs, int nsub, int lane, const double K[9], const double kd[12], double param[6], double *image_error)
{
    MpLds &s = rs->m;
    const int npts = 4 * nsub;
    // ---- (2) planarity
    double Mc[3] = {0, 0, 0}, W[3], Vt[3][3];
    {
        for (int p = lane; p < npts; p += 64) {
            const int q = RB_Q(p);
            for (int a = 0; a < 3; a++) Mc[a] += s.obj[q][a];
        }
        for (int a = 0; a < 3; a++) Mc[a] = wave_sum_f64(Mc[a]) / npts;
        double m6[6] = {0, 0, 0, 0, 0, 0};
        for (int p = lane; p < npts; p += 64) {
            const int q = RB_Q(p);
            const double d[3] = {s.obj[q][0] - Mc[0], s.obj[q][1] - Mc[1], s.obj[q][2] - Mc[2]};
            m6[0] += d[0] * d[0]; m6[1] += d[0] * d[1]; m6[2] += d[0] * d[2];
            m6[3] += d[1] * d[1]; m6[4] += d[1] * d[2]; m6[5] += d[2] * d[2];
        }
        for (int i = 0; i < 6; i++) m6[i] = wave_sum_f64(m6[i]);
        double MM[3][3] = {{m6[0], m6[1], m6[2]}, {m6[1], m6[3], m6[4]}, {m6[2], m6[4], m6[5]}};
        pnp_scatter_eig(MM, W, Vt);
    }
    const bool planar = W[2] / W[1] < 1e-3;
    // ---- (3) the start
    for (int i = 0; i < 6; i++) param[i] = 0.;
    if (planar) {
        double Rt[9], tt[3];
        pnp_plane_frame(Vt, Mc, Rt, tt);
        SR_LDS_SYNC();  // (the Mxy of the solve before this one has been read)
        for (int p = lane; p < npts; p += 64) {
            const double *src = s.obj[RB_Q(p)];
            s.Mxy[p][0] = (float)(Rt[0] * src[0] + Rt[1] * src[1] + Rt[2] * src[2] + tt[0]);
            s.Mxy[p][1] = (float)(Rt[3] * src[0] + Rt[4] * src[1] + Rt[5] * src[2] + tt[1]);
        }
        SR_LDS_SYNC();
        double h[9], R[9];
        if (rb_homography_dlt(rs, npts, lane, h)) {
            double t3[3];
            pnp_pose_from_h(h, t3);
            for (int i = 0; i < 3; i++) param[3 + i] = h[i * 3] * tt[0] + h[i * 3 + 1] * tt[1] + h[i * 3 + 2] * tt[2] + t3[i];
            pnp_mul3(h, Rt, R);
        } else {
            for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1. : 0.;
        }
        rodrigues_m2v(R, param);
    } else {
        // the subset's marker with the largest image area, the first of equals (positions in the subset, as k_map_pose's are in its list)
        int big = lane < nsub ? lane : 0;
        double abig = s.area[rs->sub[big]];
        for (int k = lane + 64; k < nsub; k += 64)
            if (s.area[rs->sub[k]] > abig) {
                abig = s.area[rs->sub[k]];
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
        const int b4 = 4 * (int)rs->sub[big];
        const double *c0 = s.obj[b4], *c2 = s.obj[b4 + 2];
        const double cc[3] = {0.5 * (c0[0] + c2[0]), 0.5 * (c0[1] + c2[1]), 0.5 * (c0[2] + c2[2])};
        pnp_start_largest<MODEL>(c0, s.obj[b4 + 1], s.obj[b4 + 3], cc, s.img + b4, K, kd, param);
    }
    // ---- (4) CvLevMarq over the 2 * npts residuals, lane l owns residuals l, l + 64, ...
    const int nres = 2 * npts;
    double S[21], gJ[6], e2 = 0;
    bool needJ = true;
    LevMarq lm;
    do {
        double Sp[21], gp[6];
        e2 = 0;
        for (int i = 0; i < 21; i++) Sp[i] = 0.;
        for (int i = 0; i < 6; i++) gp[i] = 0.;
        for (int r = lane; r < nres; r += 64) {
            const int p = RB_Q(r >> 1), sel = r & 1;
            const double M[3] = {s.obj[p][0], s.obj[p][1], s.obj[p][2]};
            double Jrow[6];
            const double err = project_one<MODEL>(M, param, K, kd, sel, Jrow, needJ) - s.img[p][sel];
            e2 += err * err;
            if (needJ) {
                int idx = 0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int c = a; c < 6; c++) Sp[idx++] += Jrow[a] * Jrow[c];
                    gp[a] += Jrow[a] * err;
                }
            }
        }
        if (needJ) {
#pragma unroll
            for (int i = 0; i < 21; i++) S[i] = wave_sum_f64(Sp[i]);
#pragma unroll
            for (int i = 0; i < 6; i++) gJ[i] = wave_sum_f64(gp[i]);
        }
    } while (lm.step(param, S, gJ, [&] { return wave_sum_f64(e2); }, needJ));
    // ---- getReprojectionError over the subset's points
    double tot = 0;
    for (int p = lane; p < npts; p += 64) {
        const int q = RB_Q(p);
        const double M[3] = {s.obj[q][0], s.obj[q][1], s.obj[q][2]};
        double Jrow[6];
        const double dx = s.img[q][0] - (double)(float)project_one<MODEL>(M, param, K, kd, 0, Jrow, false);
        const double dy = s.img[q][1] - (double)(float)project_one<MODEL>(M, param, K, kd, 1, Jrow, false);
        const double e = sqrt(dx * dx + dy * dy);
        tot += e * e;
    }
    tot = wave_sum_f64(tot);
    *image_error = tot / npts;
}
#undef RB_Q

__device__ __forceinline__ void rb_zero_pose(fid_map_pose_out *o)
{
    o->n_markers = 0;
    o->n_over = 0;
    for (int i = 0; i < 3; i++) o->rvec[i] = o->tvec[i] = o->cam_t[i] = 0.;
    for (int i = 0; i < 9; i++) o->R[i] = o->cam_R[i] = 0.;
    o->image_error = 0.;
}

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
    int nm = nmark_per_frame[(long long)f * nmark_stride_ints];
    nm = nm < 0 ? 0 : (nm > per_frame ? per_frame : nm);
    map_n = map_n > FID_MAP_MAX_ENTRIES ? FID_MAP_MAX_ENTRIES : map_n;
    // ---- (1) the frame's markers that the map names, in list order, without the ids seen twice (k_map_pose's gather)
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
            fid_map_pose_out o;
            rb_zero_pose(&o);
            out[f] = o;
            rout[f] = ro;
        }
        return;
    }
    SR_LDS_SYNC();
    const int npts = 4 * found;
    for (int p = lane; p < npts; p += 64) {
        const int k = p >> 2, q = p & 3;
        const fid_marker *mk = mlist + s.mk[k];
        const double *src = map_obj + (size_t)s.ent[k] * 12 + q * 3;
        for (int a = 0; a < 3; a++) s.obj[p][a] = src[a];
        s.img[p][0] = (double)mk->corners[2 * q];
        s.img[p][1] = (double)mk->corners[2 * q + 1];
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
    for (int p = lane; p < npts; p += 64) {
        double x, y;
        (void)pnp_undistort<MODEL>(K, kd, s.img[p][0], s.img[p][1], &x, &y);
        s.mn[p][0] = (float)x;
        s.mn[p][1] = (float)y;
    }
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
            rb_solve<MODEL>(&rs, nI, lane, K, kd, param, &image_error);
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
            rb_zero_pose(&o);
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
    const size_t n = (size_t)(c->lim.max_batch + 1);
    if (!c->d_rposes) HIPCHK(c, hipMalloc((void **)&c->d_rposes, sizeof(fid_map_pose_out) * n));
    if (!c->d_mrob) HIPCHK(c, hipMalloc((void **)&c->d_mrob, sizeof(fid_map_robust_out) * n));
    if (!c->h_rposes) HIPCHK(c, hipHostMalloc((void **)&c->h_rposes, sizeof(fid_map_pose_out) * n, hipHostMallocDefault));
    if (!c->h_mrob) HIPCHK(c, hipHostMalloc((void **)&c->h_mrob, sizeof(fid_map_robust_out) * n, hipHostMallocDefault));
    return FID_OK;
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
    fid_status rca = stage_map_markers(c, markers, n, &d_n);
    if (rca == FID_OK) rca = ensure_map_robust(c);
    if (rca != FID_OK) return rca;
    fid_map_pose_out *d_out = c->d_rposes + c->lim.max_batch;  // (the slot behind a batch's: the last call's results stay)
    fid_map_robust_out *d_rout = c->d_mrob + c->lim.max_batch;
    map_pose_robust_launch(c, c->stream, c->d_map_in, d_n, 0, n > 0 ? n : 1, 1, *camera, *opts, d_out, d_rout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(pose_out, d_out, sizeof(fid_map_pose_out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(robust_out, d_rout, sizeof(fid_map_robust_out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FID_OK;
}
