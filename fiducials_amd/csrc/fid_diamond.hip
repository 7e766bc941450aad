// fid_diamond.hip -- ChArUco diamonds (fid_abi.h: "ChArUco diamonds"): the search for four markers around one chessboard square among the
// markers of a frame, their four chessboard corners, the refinement and the pose.  Part of the fid_api.hip translation unit, behind
// fid_calib_points.hip.  Nothing here is on the detect path: a context that never asks allocates and launches nothing of it.
//
// k_diamond_propose, blockIdx.y = the frame, blockIdx.x = sixteen anchors: step 1 of the header.  The frame's marker corners are staged
//   once in LDS (256 markers: 8 KB).  A lane is (anchor, quarter): the four lanes of an anchor all hold its q_k (72 floats of arithmetic,
//   cheaper than handing them round) and each scans the candidates j = quarter, quarter + 4, ... in ascending order, so that within a
//   lane the strict < keeps the lowest j of equal distances; the four are then merged by the lexicographic minimum of (d2, j), which is
//   associative and commutative: the order of the merge cannot change the result.  A candidate enters the comparison for k only when
//   its corner 0 lies within tol_a of q_k[0] -- d2 is a maximum over the corners, so any other candidate has d2 >= tol_a^2 and could
//   only be the argmin of a proposal that is not valid anyway.  Sixteen anchors a wave: 256 markers are sixteen waves a frame.
// k_diamond_resolve, one wave per frame (blockIdx.x: a batch is one launch): step 2, the serial pass, on wave-uniform values -- the
//   proposals sit in the lanes' registers and are read by lane index, the assigned flags are four 64-bit words -- and diamond t's
//   founder is noted in lane t.  Steps 3 and 5: lanes are (diamond, corner) items, 64 at a time; the reported diamonds are compacted in
//   anchor order by ballot and prefix count.  The corner items are fid_charuco_corner records, so that step 4 is k_charuco_subpix as it
//   stands (slot = 4 diamond + corner, out_stride = 4 FID_DIAMOND_MAX_PER_FRAME).
// The pose is fid_pose_cam's road on {ids[0], corners}: no kernel here.

#define DM_MAX_MARKERS FID_DIAMOND_MAX_MARKERS
#define DM_MAX FID_DIAMOND_MAX_PER_FRAME
#define DM_SUB 4              // lanes that share an anchor's candidates
#define DM_ANCH (64 / DM_SUB)  // anchors a wave
#define DM_ITEMS (4 * DM_MAX)  // corner items a frame
#define DM_FETCH_FIRST 8       // diamonds a frame that the first copy brings back
static_assert(DM_MAX_MARKERS <= 256, "a proposal packs three list positions into bytes");
static_assert(DM_MAX * 4 >= DM_MAX_MARKERS && DM_MAX == 64, "diamond t's founder is noted in lane t");

// the layout L(rate): marker k's square is (sqx, sqy) = (1,0), (0,1), (2,1), (1,2); its four corners, rounded through float
__device__ __forceinline__ void dm_marker_obj(double s, int k, double ox[4], double oy[4])
{
    const int sqx = (0x1201 >> (4 * k)) & 3, sqy = (0x2110 >> (4 * k)) & 3;
    const double d = (s - 1.) / 2, c0x = sqx * s + d, c0y = sqy * s + d + 1.;
    ox[0] = ox[3] = (double)(float)c0x;
    ox[1] = ox[2] = (double)(float)(c0x + 1.);
    oy[0] = oy[1] = (double)(float)c0y;
    oy[2] = oy[3] = (double)(float)(c0y - 1.);
}

// rule 2's homography layout plane -> image of a marker with the plane corners (ox, oy) and the image corners ic, the centre folded in
__device__ __forceinline__ bool dm_homography(const double ox[4], const double oy[4], const float ic[8], double h[9])
{
    const double ix[4] = {(double)ic[0], (double)ic[2], (double)ic[4], (double)ic[6]};
    const double iy[4] = {(double)ic[1], (double)ic[3], (double)ic[5], (double)ic[7]};
    const double wx = ox[1] - ox[0], wy = oy[0] - oy[3];
    const double ccx = 0.5 * (ox[0] + ox[2]), ccy = 0.5 * (oy[0] + oy[2]);
    bool ok = pnp_quad_homography(ix, iy, 1. / wx, 1. / wy, h);
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && h[i] - h[i] == 0.;
#pragma unroll
    for (int r = 0; r < 3; r++) h[3 * r + 2] = h[3 * r + 2] - h[3 * r] * ccx - h[3 * r + 1] * ccy;
    return ok;
}

__device__ __forceinline__ void dm_map(const double h[9], double X, double Y, float *x, float *y)
{
    const double w = h[6] * X + h[7] * Y + h[8];
    *x = (float)((h[0] * X + h[1] * Y + h[2]) / w);
    *y = (float)((h[3] * X + h[4] * Y + h[5]) / w);
}

__device__ __forceinline__ double dm_dist2(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    return (double)dx * dx + (double)dy * dy;
}

// ------------------------------------------------------------------------------------------------ k_diamond_propose: step 1
// prop[f * prop_stride + a] = m_1 | m_2 << 8 | m_3 << 16 | 1 << 24 for a valid proposal, else 0
__global__ __launch_bounds__(64) void k_diamond_propose(const fid_marker *__restrict__ markers, const int *__restrict__ nmark_per_frame, int nmark_stride_ints,
                                                         int per_frame, double rate, double max_rep_rate, int *__restrict__ prop, int prop_stride)
{
    __shared__ __attribute__((aligned(16))) float s_c[DM_MAX_MARKERS][8];
    const int f = blockIdx.y, lane = threadIdx.x, a0 = blockIdx.x * DM_ANCH;
    const fid_marker *mlist = markers + (long long)f * per_frame;
    int nm = nmark_per_frame[(long long)f * nmark_stride_ints];
    const int room = per_frame < DM_MAX_MARKERS ? per_frame : DM_MAX_MARKERS;
    nm = nm < 0 ? 0 : (nm > room ? room : nm);
    if (a0 >= nm) return;  // (wave-uniform)
    {
        const float *src = reinterpret_cast<const float *>(mlist);  // a fid_marker is nine 4-byte words: the id, then the corners
        float *dst = &s_c[0][0];
        for (int e = lane; e < nm * 8; e += 64) dst[e] = src[(e >> 3) * 9 + 1 + (e & 7)];
    }
    __syncthreads();
    const int a = a0 + lane / DM_SUB, sub = lane % DM_SUB;
    const bool active = a < nm;
    const int ar = active ? a : a0;
    float ca[8];
#pragma unroll
    for (int i = 0; i < 8; i++) ca[i] = s_c[ar][i];
    double ox[4], oy[4], h[9];
    dm_marker_obj(rate, 0, ox, oy);
    bool ok = dm_homography(ox, oy, ca, h) && active;
    double side = 0.;
#pragma unroll
    for (int c = 0; c < 4; c++) side += sqrt(dm_dist2(ca[2 * c], ca[2 * c + 1], ca[2 * ((c + 1) & 3)], ca[2 * ((c + 1) & 3) + 1]));
    const double tol = max_rep_rate * (side / 4.), tol2 = tol * tol;
    float qx[3][4], qy[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        dm_marker_obj(rate, k + 1, ox, oy);
#pragma unroll
        for (int c = 0; c < 4; c++) dm_map(h, ox[c], oy[c], &qx[k][c], &qy[k][c]);
    }
    double best[3] = {tol2, tol2, tol2};
    int bj[3] = {INT_MAX, INT_MAX, INT_MAX};
    if (ok) {
        for (int j = sub; j < nm; j += DM_SUB) {
            if (j == a) continue;
            const float4 c01 = *reinterpret_cast<const float4 *>(&s_c[j][0]), c23 = *reinterpret_cast<const float4 *>(&s_c[j][4]);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double d2 = dm_dist2(qx[k][0], qy[k][0], c01.x, c01.y);
                if (!(d2 < tol2)) continue;
                d2 = fmax(d2, dm_dist2(qx[k][1], qy[k][1], c01.z, c01.w));
                d2 = fmax(d2, dm_dist2(qx[k][2], qy[k][2], c23.x, c23.y));
                d2 = fmax(d2, dm_dist2(qx[k][3], qy[k][3], c23.z, c23.w));
                if (d2 < best[k]) {
                    best[k] = d2;
                    bj[k] = j;
                }
            }
        }
    }
    // the anchor's four lanes: the lexicographic minimum of (d2, j)
#pragma unroll
    for (int mask = 1; mask < DM_SUB; mask <<= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double od = __shfl_xor(best[k], mask, WAVE);
            const int oj = __shfl_xor(bj[k], mask, WAVE);
            if (od < best[k] || (od == best[k] && oj < bj[k])) {
                best[k] = od;
                bj[k] = oj;
            }
        }
    }
    if (active && sub == 0) {
        const bool valid = ok && bj[0] != INT_MAX && bj[1] != INT_MAX && bj[2] != INT_MAX && bj[0] != bj[1] && bj[0] != bj[2] && bj[1] != bj[2];
        prop[(long long)f * prop_stride + a] = valid ? (bj[0] | bj[1] << 8 | bj[2] << 16 | 1 << 24) : 0;
    }
}

// ------------------------------------------------------------------------------------------------ k_diamond_resolve: steps 2, 3, 5
struct DmHead {
    int ids[4], index[4];
};

__global__ __launch_bounds__(64) void k_diamond_resolve(const fid_marker *__restrict__ markers, const int *__restrict__ nmark_per_frame, int nmark_stride_ints,
                                                         int per_frame, double rate, const int *__restrict__ prop, int prop_stride, int W, int H,
                                                         DmHead *__restrict__ heads, fid_charuco_corner *__restrict__ items, int *__restrict__ n_items)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const fid_marker *mlist = markers + (long long)f * per_frame;
    int nm = nmark_per_frame[(long long)f * nmark_stride_ints];
    const int room = per_frame < DM_MAX_MARKERS ? per_frame : DM_MAX_MARKERS;
    nm = nm < 0 ? 0 : (nm > room ? room : nm);
    // ---- step 2: the serial pass.  Lane l holds the proposals of the anchors l, l + 64, l + 128, l + 192.
    const int *pf = prop + (long long)f * prop_stride;
    int pv[DM_MAX_MARKERS / 64];
#pragma unroll
    for (int b = 0; b < DM_MAX_MARKERS / 64; b++) pv[b] = 64 * b + lane < nm ? pf[64 * b + lane] : 0;
    unsigned long long A0 = 0ull, A1 = 0ull, A2 = 0ull, A3 = 0ull;  // assigned, by list position
    auto taken = [&](int m) { return (int)(((m < 64 ? A0 : m < 128 ? A1 : m < 192 ? A2 : A3) >> (m & 63)) & 1ull); };
    auto take = [&](int m) {
        const unsigned long long bit = 1ull << (m & 63);
        A0 |= m < 64 ? bit : 0ull;
        A1 |= m >= 64 && m < 128 ? bit : 0ull;
        A2 |= m >= 128 && m < 192 ? bit : 0ull;
        A3 |= m >= 192 ? bit : 0ull;
    };
    int nd = 0, my_a = 0, my_p = 0;  // lane t: diamond t's anchor and proposal
#pragma unroll
    for (int b = 0; b < DM_MAX_MARKERS / 64; b++) {
        const int lim = nm - 64 * b < 64 ? nm - 64 * b : 64;
        for (int l = 0; l < lim; l++) {
            const int p = __builtin_amdgcn_readlane(pv[b], l), a = 64 * b + l;
            if (!(p >> 24)) continue;
            const int m1 = p & 255, m2 = (p >> 8) & 255, m3 = (p >> 16) & 255;
            if (taken(a) | taken(m1) | taken(m2) | taken(m3)) continue;
            if (nd >= DM_MAX) continue;
            take(a);
            take(m1);
            take(m2);
            take(m3);
            if (lane == nd) {
                my_a = a;
                my_p = p;
            }
            nd++;
        }
    }
    // ---- steps 3 and 5: lanes are (diamond, corner of the record) items
    const double s = rate;
    int kept = 0;
    DmHead *hdst = heads + (long long)f * DM_MAX;
    fid_charuco_corner *idst = items + (long long)f * DM_ITEMS;
    for (int t0 = 0; t0 < nd; t0 += 16) {
        const int t = t0 + (lane >> 2), r = lane & 3;
        const int ta = __shfl(my_a, t & 63, WAVE), tp = __shfl(my_p, t & 63, WAVE);
        bool keep = false;
        float x0 = 0.f, y0 = 0.f;
        int win = 1;
        const int idx[4] = {ta, tp & 255, (tp >> 8) & 255, (tp >> 16) & 255};
        if (t < nd) {
            // the record's corner r is chessboard corner i = 2, 3, 1, 0; its nearest markers kA < kB and their nearest corners
            const int i = (0x0132 >> (4 * r)) & 3;
            const int kk[2] = {(0x2100 >> (4 * i)) & 3, (0x3321 >> (4 * i)) & 3}, cn[2] = {(0x0110 >> (4 * i)) & 3, (0x2332 >> (4 * i)) & 3};
            const double X = (double)(float)(((i & 1) + 1) * s), Y = (double)(float)(((i >> 1) + 1) * s);
            float px[2], py[2];
            double minDist = -1.;
            bool ok = true;
#pragma unroll
            for (int w = 0; w < 2; w++) {
                const int m = kk[w] == 0 ? idx[0] : kk[w] == 1 ? idx[1] : kk[w] == 2 ? idx[2] : idx[3];
                const float *icp = mlist[m].corners;
                float ic[8];
#pragma unroll
                for (int q = 0; q < 8; q++) ic[q] = icp[q];
                double ox[4], oy[4], h[9];
                dm_marker_obj(s, kk[w], ox, oy);
                ok = dm_homography(ox, oy, ic, h) && ok;
                dm_map(h, X, Y, &px[w], &py[w]);
            }
            x0 = (px[0] + px[1]) / 2.f;
            y0 = (py[0] + py[1]) / 2.f;
#pragma unroll
            for (int w = 0; w < 2; w++) {
                const int m = kk[w] == 0 ? idx[0] : kk[w] == 1 ? idx[1] : kk[w] == 2 ? idx[2] : idx[3];
                const float *icp = mlist[m].corners;
                const double dist = sqrt(dm_dist2(x0, y0, icp[2 * cn[w]], icp[2 * cn[w] + 1]));
                if (minDist == -1. || dist < minDist) minDist = dist;
            }
            const double wd = minDist - 2.;
            win = !(wd >= 1.) ? 1 : (wd >= (double)CH_MAXWIN ? CH_MAXWIN : (int)wd);
            keep = ok && x0 >= 2.f && x0 < (float)(W - 2) && y0 >= 2.f && y0 < (float)(H - 2);
        }
        const unsigned long long hit = __ballot(keep);
        const bool whole = ((hit >> (lane & ~3)) & 15ull) == 15ull;  // all four corners of the lane's diamond are selected
        const unsigned long long lead = __ballot(whole && r == 0);
        if (whole) {
            const int pos = kept + __builtin_popcountll(lead & ((1ull << (lane & ~3)) - 1ull));
            fid_charuco_corner rec;
            rec.id = r;
            rec.win = win;
            rec.x = rec.x0 = x0;
            rec.y = rec.y0 = y0;
            idst[4 * pos + r] = rec;
            hdst[pos].index[r] = idx[r == 0 ? 0 : r == 1 ? 1 : r == 2 ? 2 : 3];
            hdst[pos].ids[r] = mlist[r == 0 ? idx[0] : r == 1 ? idx[1] : r == 2 ? idx[2] : idx[3]].id;
        }
        kept += __builtin_popcountll(lead);
    }
    if (lane == 0) n_items[f] = 4 * kept;
}

// ------------------------------------------------------------------------------------------------ host
// everything diamonds need on a context (nothing of it exists until the first call): the proposals, max_batch + 1 frames of results (the
// slot behind a batch's serves fid_diamonds_detect), the window masks, staging
struct DiamondBufs {
    int *d_prop = nullptr, *d_n = nullptr;
    DmHead *d_heads = nullptr;
    fid_charuco_corner *d_items = nullptr;
    float *d_mask = nullptr;
    fid_marker *d_in = nullptr;  // DM_MAX_MARKERS markers and their count
    int *d_nin = nullptr;
    DevBlock mem;  // everything above
    DevArray<uint8_t> img;
    std::vector<DmHead> h_heads;
    std::vector<fid_charuco_corner> h_items;
    std::vector<int> h_n;
};

static void diamond_free(fid_ctx *c)
{
    delete c->diamond;
    c->diamond = nullptr;
}

void fid_default_diamond_opts(fid_diamond_opts *o)
{
    if (!o) return;
    o->square_marker_rate = 0.04 / 0.024;
    o->max_rep_rate = 1.0;
    o->refine = 1;
    o->reserved0 = 0;
}

static bool diamond_refusals(fid_ctx *c, const fid_diamond_opts *o)
{
    if (!o) {
        c->last_error = "diamonds: opts is NULL";
        return true;
    }
    if (!(o->square_marker_rate - o->square_marker_rate == 0) || !(o->square_marker_rate > 1.)) {
        c->last_error = "diamonds: square_marker_rate " + std::to_string(o->square_marker_rate) + " must be finite and above 1";
        return true;
    }
    if (!(o->max_rep_rate - o->max_rep_rate == 0) || !(o->max_rep_rate > 0.)) {
        c->last_error = "diamonds: max_rep_rate " + std::to_string(o->max_rep_rate) + " must be finite and above 0";
        return true;
    }
    return refuse_in_flight(c);
}

static fid_status diamond_ensure(fid_ctx *c)
{
    if (c->diamond) return FID_OK;
    DiamondBufs *B = new (std::nothrow) DiamondBufs;
    if (!B) return FID_E_OUT_OF_MEMORY;
    const size_t slots = (size_t)c->lim.max_batch + 1;
    MemLayout l;
    l.add(&B->d_prop, DM_MAX_MARKERS * slots), l.add(&B->d_n, slots), l.add(&B->d_heads, DM_MAX * slots), l.add(&B->d_items, DM_ITEMS * slots);
    l.add(&B->d_mask, CH_MASK_STRIDE * CH_MAXWIN), l.add(&B->d_in, DM_MAX_MARKERS), l.add(&B->d_nin, 1);
    const std::vector<float> mask = charuco_subpix_masks();
    hipError_t e = B->mem.reserve(l.bytes());
    if (e == hipSuccess) {
        l.bind(B->mem.p);
        e = hipMemcpy(B->d_mask, mask.data(), mask.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) delete B;
    HIPCHK(c, e);
    c->diamond = B;  // (published when all of it exists)
    return FID_OK;
}

// the two kernels (and k_charuco_subpix) for R.F frames on the context's stream; R.per_frame <= DM_MAX_MARKERS
static fid_status diamond_enqueue(fid_ctx *c, const fid_diamond_opts &o, const ChRun &R)
{
    DiamondBufs *B = c->diamond;
    int *d_prop = B->d_prop + (size_t)R.slot0 * DM_MAX_MARKERS, *d_n = B->d_n + R.slot0;
    fid_charuco_corner *d_items = B->d_items + (size_t)R.slot0 * DM_ITEMS;
    hipLaunchKernelGGL(k_diamond_propose, dim3((R.per_frame + DM_ANCH - 1) / DM_ANCH, R.F), dim3(64), 0, c->stream, R.d_markers, R.d_nmark, R.nmark_stride_ints,
                       R.per_frame, o.square_marker_rate, o.max_rep_rate, d_prop, DM_MAX_MARKERS);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_diamond_resolve, dim3(R.F), dim3(64), 0, c->stream, R.d_markers, R.d_nmark, R.nmark_stride_ints, R.per_frame, o.square_marker_rate,
                       (const int *)d_prop, DM_MAX_MARKERS, R.W, R.H, B->d_heads + (size_t)R.slot0 * DM_MAX, d_items, d_n);
    HIPCHK(c, hipGetLastError());
    if (o.refine) {
        hipLaunchKernelGGL(k_charuco_subpix, dim3(DM_ITEMS, R.F), dim3(64), 0, c->stream, R.gray, R.gfstride, R.gs, R.W, R.H, d_items, DM_ITEMS, (const int *)d_n,
                           (const float *)B->d_mask);
        HIPCHK(c, hipGetLastError());
    }
    return FID_OK;
}

// the records of F frames from slot0 on, into out (cap diamonds a frame): FID_E_CAPACITY where a frame holds more
static fid_status diamond_fetch(fid_ctx *c, int slot0, int F, fid_diamond *out, int cap, int32_t *n_per_frame)
{
    DiamondBufs *B = c->diamond;
    B->h_n.resize((size_t)F);
    B->h_heads.resize((size_t)F * DM_MAX);
    B->h_items.resize((size_t)F * DM_ITEMS);
    HIPCHK(c, hipMemcpyAsync(B->h_n.data(), B->d_n + slot0, sizeof(int) * (size_t)F, hipMemcpyDeviceToHost, c->stream));
    // a frame seldom holds more than a few diamonds: the first DM_FETCH_FIRST of every frame come with the counts (two strided copies,
    // 1 KB a frame in place of 8 KB); only a call with a fuller frame goes back for the rest
    const DmHead *sh = B->d_heads + (size_t)slot0 * DM_MAX;
    const fid_charuco_corner *si = B->d_items + (size_t)slot0 * DM_ITEMS;
    HIPCHK(c, hipMemcpy2DAsync(B->h_heads.data(), sizeof(DmHead) * DM_MAX, sh, sizeof(DmHead) * DM_MAX, sizeof(DmHead) * DM_FETCH_FIRST, (size_t)F,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(B->h_items.data(), sizeof(fid_charuco_corner) * DM_ITEMS, si, sizeof(fid_charuco_corner) * DM_ITEMS,
                               sizeof(fid_charuco_corner) * 4 * DM_FETCH_FIRST, (size_t)F, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool fuller = false;
    for (int f = 0; f < F; f++) fuller = fuller || B->h_n[(size_t)f] > 4 * DM_FETCH_FIRST;
    if (fuller) {
        HIPCHK(c, hipMemcpyAsync(B->h_heads.data(), sh, sizeof(DmHead) * (size_t)F * DM_MAX, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(B->h_items.data(), si, sizeof(fid_charuco_corner) * (size_t)F * DM_ITEMS, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    fid_status rc = FID_OK;
    for (int f = 0; f < F; f++) {
        int n = B->h_n[(size_t)f] / 4;
        n = n < 0 ? 0 : (n > DM_MAX ? DM_MAX : n);
        n_per_frame[f] = n;
        if (n > cap) {
            c->last_error = "caller room for " + std::to_string(cap) + " diamonds a frame, frame " + std::to_string(f) + " has " + std::to_string(n);
            rc = FID_E_CAPACITY;
        }
        const int m = n < cap ? n : cap;
        for (int t = 0; t < m; t++) {
            fid_diamond &d = out[(size_t)f * cap + t];
            const DmHead &hd = B->h_heads[(size_t)f * DM_MAX + t];
            for (int r = 0; r < 4; r++) {
                const fid_charuco_corner &it = B->h_items[(size_t)f * DM_ITEMS + 4 * t + r];
                d.ids[r] = hd.ids[r];
                d.index[r] = hd.index[r];
                d.corners[2 * r] = it.x;
                d.corners[2 * r + 1] = it.y;
                d.corners0[2 * r] = it.x0;
                d.corners0[2 * r + 1] = it.y0;
                d.win[r] = it.win;
            }
        }
    }
    return rc;
}

fid_status fid_diamonds_last(fid_ctx *c, const fid_diamond_opts *opts, fid_diamond *out, int32_t cap_per_frame, int32_t *n_per_frame)
{
    if (!c) return FID_E_INVALID_ARG;
    if (!n_per_frame || cap_per_frame < 0 || (cap_per_frame > 0 && !out)) {
        c->last_error = "diamonds: a NULL output (out with cap_per_frame > 0, n_per_frame), or cap_per_frame < 0";
        return FID_E_INVALID_ARG;
    }
    if (diamond_refusals(c, opts)) return FID_E_INVALID_ARG;
    if (c->last_frames <= 0) {
        c->last_error = "diamonds: no last call (fid_detect* or fid_collect first)";
        return FID_E_INVALID_ARG;
    }
    if (c->P.maxMarkers > DM_MAX_MARKERS) {
        c->last_error = "diamonds: the context's max_markers_per_frame " + std::to_string(c->P.maxMarkers) + " exceeds FID_DIAMOND_MAX_MARKERS (" +
                        std::to_string(DM_MAX_MARKERS) + ")";
        return FID_E_UNSUPPORTED;
    }
    HIPCHK(c, hipSetDevice(c->device));
    fid_status rc = diamond_ensure(c);
    if (rc != FID_OK) return rc;
    const ChRun R = charuco_last_frames(c);
    rc = diamond_enqueue(c, *opts, R);
    if (rc != FID_OK) return rc;
    return diamond_fetch(c, 0, c->last_frames, out, cap_per_frame, n_per_frame);
}

fid_status fid_diamonds_detect(fid_ctx *c, const fid_diamond_opts *opts, const fid_marker *markers, int32_t n, const uint8_t *img, int32_t width,
                               int32_t height, int32_t stride_bytes, fid_diamond *out, int32_t cap, int32_t *n_out)
{
    if (!c) return FID_E_INVALID_ARG;
    if (!n_out || cap < 0 || (cap > 0 && !out) || n < 0 || (n > 0 && !markers) || !img) {
        c->last_error = "diamonds: a NULL argument (out with cap > 0, n_out, markers with n > 0, img), or a negative count";
        return FID_E_INVALID_ARG;
    }
    if (width < 8 || height < 8 || stride_bytes < width || width > c->lim.max_width || height > c->lim.max_height) {
        c->last_error = "diamonds: an image of " + std::to_string(width) + " x " + std::to_string(height) + " (stride " + std::to_string(stride_bytes) +
                        ") is outside the context's frame limits";
        return FID_E_INVALID_ARG;
    }
    if (diamond_refusals(c, opts)) return FID_E_INVALID_ARG;
    if (n > DM_MAX_MARKERS) {
        c->last_error = "diamonds: " + std::to_string(n) + " markers, at most FID_DIAMOND_MAX_MARKERS (" + std::to_string(DM_MAX_MARKERS) + ")";
        return FID_E_UNSUPPORTED;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const fid_status rce = diamond_ensure(c);
    if (rce != FID_OK) return rce;
    DiamondBufs *B = c->diamond;
    fid_status rcs = stage_gray(c, B->img, img, width, height, stride_bytes);
    if (rcs == FID_OK) rcs = upload_markers(c, B->d_in, B->d_nin, markers, n);
    if (rcs != FID_OK) return rcs;
    const int slot = c->lim.max_batch;
    const ChRun R = {B->d_in, B->d_nin, 0, n > 0 ? n : 1, 1, B->img.data(), 0, width, width, height, slot};
    const fid_status rc = diamond_enqueue(c, *opts, R);
    if (rc != FID_OK) return rc;
    return diamond_fetch(c, slot, 1, out, cap, n_out);
}

fid_status fid_diamond_pose_cam(fid_ctx *c, const fid_camera *camera, const fid_diamond *diamonds, int32_t n, double square_len, fid_pose_out *out)
{
    if (!c || n < 0 || (n > 0 && (!diamonds || !out))) return FID_E_INVALID_ARG;
    std::vector<fid_marker> mk((size_t)n);
    std::vector<double> lens((size_t)n, square_len);
    for (int i = 0; i < n; i++) {
        mk[(size_t)i].id = diamonds[i].ids[0];
        memcpy(mk[(size_t)i].corners, diamonds[i].corners, sizeof(float) * 8);
    }
    return fid_pose_cam(c, camera, mk.data(), lens.data(), n, square_len, out);
}
