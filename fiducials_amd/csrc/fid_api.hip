// fid_api.hip -- the C-ABI of libfid_amd.so (include/fid_abi.h): context, buffers in HBM, the launch
// sequence of the detection pipeline on one HIP stream, result hand-back.  No CPU fallback: without a
// HIP device fid_create fails with FID_E_NO_DEVICE.
#include "fid_kernels.hip"

#include "fid_devmem.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

namespace {

enum { ST_GRAY = 0, ST_THRESH, ST_STARTS, ST_PROBE, ST_WALK, ST_APPROX, ST_SORT, ST_NEAR, ST_RESOLVE, ST_IDENT, ST_FILTER, ST_SUBPIX, ST_POSE, ST_SEEDWALK,
       ST_SEEDLESS, ST_COUNT };
// (cycle tracing: walk_probe / walk_full / approx are the main stream's seed walk / link + cycles + copy / approx of the seed
//  cycles; seedless_chain is the auxiliary stream's probes + survivor walk + cycles + copy + approx beside them)
const char *const kStageNames[ST_COUNT] = {"to_gray", "threshold", "find_starts", "walk_probe", "walk_full", "approx", "sort_cands",
                                           "near", "resolve", "identify", "filter_markers", "subpix", "pose", "seed_walk", "seedless_chain"};
// A sub-batch's event row (fid_ctx::sub_ev, FID_PROFILE): events 0 .. ST_SUBPIX + 1 are the stage boundaries on its main stream (stage i
// runs from event i to event i + 1); beside them the brackets of the seed walk (main stream), of the seedless chain (auxiliary
// stream) and of the remembered marker pose
enum { EV_SEEDWALK0 = 14, EV_SEEDWALK1, EV_SEEDLESS0, EV_SEEDLESS1, EV_POSE0, EV_POSE1, EV_COUNT };
static_assert(EV_SEEDWALK0 > ST_SUBPIX + 1, "the brackets lie behind the stage boundaries");

constexpr int TX = 128, TY = 32, NT = 256;
constexpr int THRW_NT = 512, THRW_WT = 16;  // k_threshold_wide: 512 threads x 16 columns cover the 8191-px frame limit
static_assert(THRW_NT * THRW_WT >= 8191, "k_threshold_wide: a row per workgroup");

}  // namespace

struct fid_ctx;

// What a fid_*_last* call asks for beside the markers of the last detect call.  The fields a kind of request does not have stay zero.
struct PoseAsk {
    fid_camera cam;             // (normalised: D beyond n_dist zero; the model is part of "the same camera")
    double len;                 // marker pose: fiducial_len
    bool cov;                   // marker pose and map pose: with the covariance ...
    double sigma;               // ... at this sigma_px
    fid_map_robust_opts opts;   // map pose by consensus: inlier_px, min_markers
};

// A remembered request: a fid_*_last* call that had to run its kernel remembers what it was asked.  The next fid_detect_* /
// fid_submit_* then runs the same kernel for it in its own stream (under the other sub-batch's tail instead of after everything, and
// without a second host round trip), and the same question after that call only hands the records over.  Same kernel, same
// arithmetic, same results.  The context holds one for the marker pose, one for the map pose, one for the map pose by consensus.
struct PoseRequest {
    enum Kind { MARKER, MAP, MAP_ROBUST };
    Kind kind;
    PoseAsk ask = {};
    bool armed = false;    // the next detect call computes it
    bool at_hand = false;  // the records in pinned host memory (the marker pose's covariances: on the device) answer it
    explicit PoseRequest(Kind k) : kind(k) {}
    // armed, and what the kernel needs is there: a map, the robust records.  enqueue_detect launches by it, finish_detect marks by it
    inline bool ahead(const fid_ctx *c) const;
    // a batch was enqueued, or the map has changed: nothing is at hand
    void forget() { at_hand = false; }
    // the batch has finished: what was computed ahead is at hand
    void finished(const fid_ctx *c) { at_hand = ahead(c); }
    // are the records at hand the answer to `a`?  (Asked without the covariance where it was remembered with one: yes, and the
    // covariance stays armed.  Asked with it where it was remembered without, or at another sigma_px: no.)
    bool answers(const PoseAsk &a) const
    {
        return at_hand && !memcmp(&ask.cam, &a.cam, sizeof a.cam) && ask.len == a.len && ask.opts.inlier_px == a.opts.inlier_px &&
               ask.opts.min_markers == a.opts.min_markers && (!a.cov || (ask.cov && ask.sigma == a.sigma));
    }
    // `a` was just computed behind the detect call: remember it, unless looking ahead is switched off (read per call: tests set it)
    void answered(const PoseAsk &a)
    {
        ask = a;
        armed = at_hand = getenv("FID_NO_POSE_AHEAD") == nullptr;
    }
};

// A marker list handed in from the host and, behind its `cap` markers, its count (stage_markers): grows in steps of 256 markers
struct MarkerStage {
    DevBlock mem;
    int cap = 0;
    fid_marker *markers() const { return (fid_marker *)mem.p; }
};

struct fid_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    enum { MAX_SUB = 8 };
    // ---- launch tunables: read from the environment once, by read_tuning() in fid_create
    struct Tuning {
        // -- how a call is cut into sub-batches and how they are ordered
        int sub_frames = 0;                    // FID_SUB_FRAMES: frames per sub-batch (0 = automatic)
        // FID_SUB_SHARES: the pieces of a resident call of 32 frames or more, per cent ("64,36" unless set; set, it also cuts a batch
        // of a chain, see plan_sub_batches).  What the text holds of positive numbers, at most MAX_SUB of them
        bool sub_shares_set = false;
        int sub_share[MAX_SUB] = {64, 36}, n_sub_share = 2;
        int feed_share[4] = {20, 30, 30, 20};  // FID_FEED_SHARES: the four copy pieces of a host-fed call (measured 15.7 k frames/s; 25-25-25-25: 15.3 k,
                                               // 34-28-22-16: 15.4 k, 10-22-34-34: 15.0 k)
        // ONE blocking call laid out like the batches in turn of two contexts (round 5): `pieces` pieces, piece k's front (threshold ..
        // approxPolyDP) on main stream k & 1, its seedless chain AND its candidate tail (sort .. pose) on auxiliary stream k & 1; piece
        // k + 1's threshold starts when piece k's find_starts is through -- four streams in all (the runtime's four hardware queues),
        // the latency-bound tail of a piece under the fronts of the pieces behind it.  0 / 1: the two sub-batches side by side.
        int pieces = 0;                        // FID_PIECES
        int stagger = 0;                       // FID_STAGGER: sub-batch k starts when sub-batch k - stagger has left its contour stage (0: all at once)
        int fs_barrier = 0;                    // FID_FS_BARRIER=1: the walks of every sub-batch wait for all find_starts (measured: find_starts
                                               // 3.6 -> 2.2 ms, the seed walks 3.3 -> 4.9 ms now side by side: the step is the same)
        // batches in turn on several contexts (fid_order_after): tail_ev is recorded where the LAST sub-batch of a batch has its
        // chip-filling kernels behind it (chain_at: 0 after find_starts, 1 seed walk, 2 copy, 3 approxPolyDP, 4 in front of the
        // candidate sort, 5 after the too-close filter)
        int chain_at = 0;                      // FID_CHAIN_AT
        bool idx_stream = true;                // FID_NO_IDX_STREAM unset: calls laid out as one piece of up to 16 frames run k_seed_index on a stream of its own
        bool prio = false;                     // FID_PRIO=1: earlier sub-batches more urgent.  Measured slower (18.1k vs 18.8k frames/s) than equal priorities.
        // -- the front
        int thr_xcd = 1;  // strips dealt out so that an XCD works through neighbouring strips (FID_THR_XCD=0: plain grid order)
        int thr_nw = 3, thr_split = 0, thr_rows = 0;  // stream kernel: consumer waves per workgroup, un-fused LDS reads, rows per workgroup (0 = automatic)
        int seed_shift = 0;        // FID_SEED_SHIFT: force the seed grid spacing 8 << shift (0 = by call size)
        int seed_kernel = 0;       // FID_SEED_KERNEL=split|fused: k_find_starts<false> + k_find_seeds, or k_find_starts<true> (0 = by the seed grid)
        // -- the contour stages
        bool trace_legacy = false;  // FID_TRACE=legacy: every call of the context is traced by the whole-border walk (fid_ctx::whole_border_walk)
        int walk_blocks = 0;  // FID_WALK_BLOCKS: one-wave workgroups per frame in the full walk pass (0 = automatic)
        int walk_blocks_cap = 0;   // FID_WALK_CAP: most walker workgroups per frame (0: 64, 256 for calls of one or two frames)
        int walk2_div = 6;   // FID_WALK2_DIV: the survivor walk gets walk_blocks / this workgroups a frame (round 6: 2 -> 6, one workgroup a frame at 128 frames: 1.5 k
                             // survivors over 4 waves instead of 12 -- 1.13 M -> 0.70 M VALU wave-instructions a frame, lane utilisation 0.24 -> 0.33, same frame rate)
        int sw_blocks = 0;   // FID_SW_BLOCKS: seed-walker workgroups per frame (0 = automatic)
        int copy_blocks = 0;  // FID_COPY_BLOCKS: workgroups per frame of k_seg_copy (0: 256; a quarter of it for the seedless chain's)
        int probe_refill = 4;  // FID_PROBE_REFILL: workgroups per frame of the refilled second probe pass (0: k_probe_lut<32, 1>)
        int probe_refill0 = 0;  // FID_PROBE_REFILL0: the same for the first pass (0: k_probe_lut<6, 0>)
        int probe_passes = 1;   // FID_PROBE_PASSES: 1: a batch sieves its starts in ONE refilled pass (k_probe_refill<32, 2>: starts -> surv, surv1 / nsurv1 unused);
                                // 2: the two passes (k_probe_lut<6, 0> + k_probe_refill<32, 1>), as calls of fewer than 16 frames always do.  Values other
                                // than 1 and 2 are ignored.  The single pass is a refilled one: FID_PROBE_REFILL=0 (no refilled kernels) takes the two
                                // passes whatever this says
        int probe_single = 16;  // FID_PROBE_SINGLE: workgroups per frame of that single pass, clamped to 1 ... 64 (8 ... 32 measured alike)
        int segc_warm = 1;      // FID_NO_SEGC_WARM unset: k_seg_cycles<48> of a call of one or two frames first reads the frame's segment table (its `warm`)
        // -- the candidate tail
        int light_x = 1;     // FID_LIGHT_X: grid multiplier of k_near / k_seg_cycles, 1024 threads for k_sort_cands
        int resolve_lds_kb = 64;   // FID_RESOLVE_LDS: KB of LDS a k_resolve workgroup asks for (see launch_grids)
        int resolve_serial = 0;    // FID_RESOLVE_SERIAL=1: k_resolve's single-wave path even when the near triangle fits LDS (tests)
        int resolve_reg_max = 64;  // FID_RESOLVE_REG_MAX: components of up to so many candidates are resolved in registers (0: none; tests)
        int tail_grid = 4096;  // FID_TAIL_GRID: workgroups of k_identify (x 4: k_subpix) -- 1024 left 5 k candidates five rounds of an 80 us chain: +5 %
        bool subpix_win7 = false;  // FID_SUBPIX_WIN7=1: windows up to 5 run k_subpix<7>, the instantiation they had before k_subpix<5> (tests, A/B)
        int filter_lds = 256;  // markers k_filter_markers keeps in LDS (FID_FILTER_LDS; more go through the global scratch)
    } tune;
    // ---- streams and the events between them
    hipStream_t sub_stream[MAX_SUB] = {};  // sub-batches of one call run on these, overlapping each other's tails
    int sub_prio[MAX_SUB] = {};
    hipStream_t aux_stream[MAX_SUB] = {};  // per sub-batch: the seed walk runs here, beside the probe passes and the survivor walk
    hipStream_t idx_stream = nullptr;      // calls laid out as ONE piece (a frame or two, a batch of a chain): k_seed_index on a stream of its own
    hipEvent_t aux_fork[MAX_SUB] = {}, aux_join[MAX_SUB] = {}, aux_idx[MAX_SUB] = {};
    hipEvent_t sub_done[MAX_SUB] = {}, fork_ev = nullptr;
    hipStream_t copy_stream = nullptr;     // fid_detect_batch: the frames go up sub-batch by sub-batch on this stream ...
    hipEvent_t in_ready[MAX_SUB] = {};     // ... and a sub-batch starts when its frames have landed (H2D of k + 1 under the compute of k)
    // batches in turn on several contexts (fid_order_after): tail_ev is recorded where the LAST sub-batch of a batch has its
    // chip-filling kernels behind it (Tuning::chain_at); the next batch's first kernel, on another context, waits for wait_ev
    hipEvent_t tail_ev = nullptr, wait_ev = nullptr;
    // host-fed batches in turn: the copy of this context's next batch starts when the copy of the batch in flight on the other
    // context has landed (wait_copy_ev = that context's in_ready event).  Two copies side by side share the link, both take
    // twice as long, and the two contexts then run in lockstep: 13.8 k frames/s from pinned memory instead of 21 k.
    hipEvent_t wait_copy_ev = nullptr;
    hipEvent_t fs_done[MAX_SUB] = {};      // a sub-batch's start / seed search is through (the piece chain, FID_FS_BARRIER)
    hipEvent_t walk_done[MAX_SUB] = {};    // a sub-batch has left its contour stage (staggered starts, FID_STAGGER)
    hipEvent_t front_done[MAX_SUB] = {};   // the piece chain: a piece's main stream is through approxPolyDP, its tail goes on on the auxiliary stream
    hipEvent_t sub_ev[MAX_SUB][EV_COUNT] = {};  // per sub-batch stage boundaries (FID_PROFILE)
    // ---- the call in progress and the batch in flight (state, not tunables: the entry points set it around enqueue_detect)
    bool blocking = false;        // the call in progress is fid_detect*: nobody can chain behind it (no tail_ev on its stream)
    bool chained = false;         // the next submit is one of a chain of batches (fid_order_after): one sub-batch, see plan_sub_batches
    bool host_feed = false;       // this call's frames go up sub-batch by sub-batch on the copy stream (feed_and_enqueue)
    bool from_host_call = false;  // enqueue_detect is running under feed_and_enqueue: the sub-batches are the copy's pieces, never a piece chain
    bool piece_chain = false;     // this call is laid out as a chain of pieces (Tuning::pieces)
    bool tail_recorded = false;   // this call has recorded tail_ev (chain_point)
    bool whole_border_walk = false;  // probe passes + whole-border walk only (FID_TRACE=legacy, and a call whose seed tables overflowed);
                                     // else cycle tracing: borders read off the seed cycles, starts only for borders without a seed
    struct Pending {                       // the batch fid_submit_device enqueued and fid_collect has not yet fetched
        const uint8_t *d_src;
        int F, W, H, stride;
        long long fstride;
        fid_encoding enc;
    } pend = {};
    bool in_flight = false;
    bool fed_from_host = false;  // the batch in flight came through feed_and_enqueue
    fid_params params;
    fid_limits lim;
    DevParams P;
    std::vector<uint8_t> dict_host;
    int dict_ms = 0, dict_maxc = 0, dict_n = 0;
    // device buffers
    DevArray<uint8_t> in;  // the frames of a call that brings them from the host (feed_and_enqueue)
    uint8_t *d_gray = nullptr;
    uint32_t *d_masks = nullptr;
    size_t masks_bytes = 0;
    int masks_W = 0, masks_H = 0, masks_S = 0;
    uint2 *d_starts = nullptr, *d_surv1 = nullptr, *d_surv = nullptr;
    uint32_t *d_pool = nullptr;
    // seed-accelerated tracing
    DevSegC *d_segs = nullptr;
    DevPend *d_pend = nullptr;
    uint2 *d_seedq = nullptr;
    unsigned long long *d_seedhash = nullptr;  // per frame: seed state -> seed index (SeedHash, fid_kernels.hip)
    int seed_hash_cap = 0, seed_gen = 0;
    uint4 *d_wres = nullptr, *d_cinfo = nullptr;
    uint32_t *d_cbase = nullptr, *d_dense = nullptr;
    uint4 *d_recs = nullptr;  // copy records: pieces of the accepted contours
    long long fallbacks = 0;  // calls that fell back to the whole-border walk because the seed table was too small
    int max_chunks = 0;
    uint4 *d_contours = nullptr;
    uint32_t *d_ckpts = nullptr;
    size_t ckpts_elems = 0;
    DevCand *d_cands = nullptr, *d_sorted = nullptr, *d_filtered = nullptr;
    float4 *d_cmeta = nullptr;
    uint32_t *d_near = nullptr;
    DevIdent *d_ident = nullptr;
    uint8_t *d_bits = nullptr;  // [max_batch][max_cands][msb^2] cell bits (FID_TAP_BITS)
    int bits_cap = 0;           // msb^2 the array has room for
    fid_marker *d_pre = nullptr, *d_markers = nullptr, *d_filter_scratch = nullptr;
    int *d_accsrc = nullptr, *d_mksrc = nullptr;  // the filtered candidate behind every identified / kept marker (k_filter_markers -> k_refine_contour)
    fid_pose_out *d_poses = nullptr;
    DevCounts *d_counts = nullptr;
    DevGlobal *d_global = nullptr;
    unsigned *d_worklist = nullptr, *d_nwork = nullptr;
    uint8_t *d_dict = nullptr;
    float *d_subpix_mask = nullptr;
    uint8_t *d_probe_tables = nullptr;  // k_probe_lut's forward and backward step tables (4 KB, built once: k_probe_tables)
    // fid_pose_cam's markers, poses and lengths: one block laid out for pose_cap markers
    DevBlock pose_mem;
    double *d_lens = nullptr;
    fid_marker *d_pose_in = nullptr;
    fid_pose_out *d_pose_out = nullptr;
    int *d_pose_n = nullptr;
    int pose_cap = 0;
    // what a call hands back -- global flags, per-frame counters, markers, poses -- lies in ONE device block and ONE pinned host
    // block, laid out for the call's frame count (layout_results): one fill at the start of a call and one copy at its end instead
    // of three fills and three or four copies (each a ~5 us kernel on the stream of a 0.8 ms single-frame call)
    uint8_t *d_res = nullptr, *h_res = nullptr;
    size_t res_clear_bytes = 0, res_markers_end = 0, res_poses_end = 0, res_poses_off = 0;
    bool res_precleared = false;  // feed_and_enqueue has put this call's clear of d_res in front of its host -> device copy
    // pinned host staging
    fid_marker *h_markers = nullptr;
    DevCounts *h_counts = nullptr;
    DevGlobal *h_global = nullptr;
    fid_pose_out *h_poses = nullptr;
    // the remembered requests (PoseRequest): fid_pose_last*: k_pose (+ k_pose_cov) at the end of every sub-batch's stream;
    // fid_map_pose_last*: k_map_pose (or its COV form) behind them; fid_map_pose_robust_last_cam: k_map_pose_robust behind the result copy
    PoseRequest pose_req{PoseRequest::MARKER}, map_req{PoseRequest::MAP}, rob_req{PoseRequest::MAP_ROBUST};
    // the pose covariance (nothing of it exists until the first _cov call): a fid_pose_cov beside every fid_pose_out of the context's
    // largest call, on the device only (a _cov call copies out what the frames' counts need)
    DevArray<fid_pose_cov> pcov;
    DevArray<fid_pose_cov> pcov_in;  // fid_pose_cov_cam's, beside d_pose_in
    // the map of fiducials (fid_set_map; nothing of it exists until the first one is set): its ids ascending, per entry the four
    // object points in the map frame; a fid_map_pose_out per frame of a batch and one more for fid_map_pose, on the device and in
    // pinned host memory; room for markers handed in from the host (stage_markers).  Each of the three groups below is one device
    // block and one pinned block that exist together or not at all (alloc_bound): its pointers are null until both do
    DevBlock map_mem, mcov_mem, rob_mem;
    PinnedBlock map_hmem, mcov_hmem, rob_hmem;
    int *d_map_ids = nullptr;
    double *d_map_obj = nullptr;
    int map_n = 0;
    fid_map_pose_out *d_mposes = nullptr, *h_mposes = nullptr;
    MarkerStage map_in;
    // as pcov, for k_map_pose_cov: max_batch + 1 records like d_mposes, allocated by the first _cov call
    fid_map_pose_cov *d_mcov = nullptr, *h_mcov = nullptr;
    // k_map_pose_robust (fid_map_pose_robust.hip): max_batch + 1 pose and robust records of its own, allocated by the first robust call
    fid_map_pose_out *d_rposes = nullptr, *h_rposes = nullptr;
    fid_map_robust_out *d_mrob = nullptr, *h_mrob = nullptr;
    // fid_calibrate_map (fid_calib.hip): its buffers, sized by the views of the largest call; nothing until the first call
    struct CalibBufs *calib = nullptr;
    // fid_build_map_cam (fid_map_build.hip): one buffer sized by the largest call; nothing until the first call
    struct BuildBufs *build = nullptr;
    // the ChArUco board (fid_charuco.hip): its tables and result slots; nothing until the first fid_set_charuco_board
    struct CharucoBufs *charuco = nullptr;
    // fid_calibrate_charuco (fid_calib_points.hip): the point tables beside `calib`; nothing until the first call
    struct CalibPtsBufs *calib_pts = nullptr;
    // ChArUco diamonds (fid_diamond.hip): proposals, result slots, staging; nothing until the first fid_diamonds_* call
    struct DiamondBufs *diamond = nullptr;
    // the camera rig (fid_rig_pose.hip): its camera table and result slots; nothing until the first fid_set_rig
    struct RigBufs *rig = nullptr;
    // last call
    int last_frames = 0, last_W = 0, last_H = 0, last_nsub = 1;
    const uint8_t *last_gray = nullptr;
    long long last_gfstride = 0;
    bool profile = false;
    hipEvent_t pose_ev[2] = {};  // FID_PROFILE: the bracket of a pose kernel on the context's stream (run_pose)
    float stage_ms[ST_COUNT] = {};
    std::string last_error;
};

inline bool PoseRequest::ahead(const fid_ctx *c) const { return armed && (kind == MARKER || c->map_n > 0) && (kind != MAP_ROBUST || c->d_mrob); }

// k_map_pose for F frames on a stream (fid_map_pose.hip, at the end of this translation unit)
static void map_pose_launch(fid_ctx *c, hipStream_t st, const fid_marker *d_markers, const int *d_n, int n_stride_ints, int per_frame, int F,
                            const fid_camera &camera, fid_map_pose_out *d_out, bool with_cov = false, double sigma_px = 0.,
                            fid_map_pose_cov *d_cov = nullptr);
// k_map_pose_robust for F frames on a stream (fid_map_pose_robust.hip, behind fid_map_pose.hip)
static void map_pose_robust_launch(fid_ctx *c, hipStream_t st, const fid_marker *d_markers, const int *d_n, int n_stride_ints, int per_frame, int F,
                                   const fid_camera &camera, const fid_map_robust_opts &opts, fid_map_pose_out *d_out, fid_map_robust_out *d_rout);

// fid_calibrate_map's buffers (fid_calib.hip, behind fid_map_pose_robust.hip)
static void calib_free(fid_ctx *c);
// fid_build_map_cam's buffer (fid_map_build.hip, behind fid_calib.hip)
static void build_free(fid_ctx *c);
// the ChArUco board's buffers (fid_charuco.hip, behind fid_map_build.hip)
static void charuco_free(fid_ctx *c);
// fid_calibrate_charuco's buffers (fid_calib_points.hip, behind fid_charuco.hip)
static void calib_pts_free(fid_ctx *c);
// the diamonds' buffers (fid_diamond.hip, behind fid_calib_points.hip)
static void diamond_free(fid_ctx *c);
// the rig's buffers (fid_rig_pose.hip, behind fid_diamond.hip)
static void rig_free(fid_ctx *c);

namespace {

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                \
            return e_ == hipErrorOutOfMemory ? FID_E_OUT_OF_MEMORY : FID_E_HIP;                   \
        }                                                                                         \
    } while (0)

template <typename T>
fid_status dalloc(fid_ctx *c, T **p, size_t count)
{
    HIPCHK(c, hipMalloc((void **)p, count * sizeof(T)));
    return FID_OK;
}

// A feature's device block and its pinned twin, both or neither: the layouts' pointers are written only when both blocks exist
fid_status alloc_bound(fid_ctx *c, DevBlock &dev, const MemLayout &dl, PinnedBlock &host, const MemLayout &hl)
{
    hipError_t e = dev.reserve(dl.bytes());
    if (e == hipSuccess) e = host.reserve(hl.bytes());
    if (e != hipSuccess) {
        dev.release();
        host.release();
    }
    HIPCHK(c, e);
    dl.bind(dev.p);
    hl.bind(host.p);
    return FID_OK;
}

// n markers and their count from the host to d_markers and d_n, on the context's stream
fid_status upload_markers(fid_ctx *c, fid_marker *d_markers, int *d_n, const fid_marker *markers, int32_t n)
{
    if (n > 0) HIPCHK(c, hipMemcpyAsync(d_markers, markers, sizeof(fid_marker) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_n, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (n is a stack temporary)
    return FID_OK;
}

// a marker list from the host in `s`, its count behind it at *d_n (the map _cam entry points, fid_charuco_interpolate_cam)
fid_status stage_markers(fid_ctx *c, MarkerStage &s, const fid_marker *markers, int32_t n, int **d_n)
{
    if (n > s.cap || !s.mem.p) {
        const int cap = (n + 256) / 256 * 256;
        s.cap = 0;
        HIPCHK(c, s.mem.reserve(sizeof(fid_marker) * (size_t)cap + sizeof(int)));
        s.cap = cap;
    }
    *d_n = (int *)(s.markers() + s.cap);
    return upload_markers(c, s.markers(), *d_n, markers, n);
}

// a gray image from the host's rows, packed (stride = width) into `img`, which grows with the largest image; on the context's stream
fid_status stage_gray(fid_ctx *c, DevArray<uint8_t> &img, const uint8_t *src, int width, int height, int stride_bytes)
{
    HIPCHK(c, img.reserve((size_t)width * height));
    HIPCHK(c, hipMemcpy2DAsync(img.data(), (size_t)width, src, (size_t)stride_bytes, (size_t)width, (size_t)height, hipMemcpyHostToDevice, c->stream));
    return FID_OK;
}

// the refusals the entry points share: true, with the message set, when the call cannot go on
bool refuse_in_flight(fid_ctx *c)
{
    if (c->in_flight) c->last_error = "a submitted batch is in flight: fid_collect first";
    return c->in_flight;
}
bool refuse_no_map(fid_ctx *c)
{
    if (c->map_n == 0) c->last_error = "no map: fid_set_map first";
    return c->map_n == 0;
}
bool refuse_room(fid_ctx *c, int cap_frames)
{
    if (cap_frames < c->last_frames)
        c->last_error = "caller room for " + std::to_string(cap_frames) + " frames, the last call had " + std::to_string(c->last_frames);
    return cap_frames < c->last_frames;
}

int roundup(int v, int m) { return (v + m - 1) / m * m; }

// [DevGlobal][nwork][DevCounts x F] (cleared at the start of a call) [fid_marker x F x MM][fid_pose_out x F x MM]: the block a call's
// results lie in, on the device and in pinned host memory; *clear_end, *markers_end: where the cleared part and the markers end
MemLayout results_layout(int F, int MM, DevGlobal **global, unsigned **nwork, DevCounts **counts, fid_marker **markers, fid_pose_out **poses,
                         size_t *clear_end = nullptr, size_t *markers_end = nullptr)
{
    MemLayout l;
    l.add(global, 1), l.add(nwork, fid_ctx::MAX_SUB), l.add(counts, (size_t)F);
    if (clear_end) *clear_end = l.mark();
    l.add(markers, (size_t)F * MM);
    if (markers_end) *markers_end = l.mark();
    l.add(poses, (size_t)F * MM);
    return l;
}
size_t results_bytes(int F, int MM)
{
    DevGlobal *g; unsigned *nw; DevCounts *cn; fid_marker *mk; fid_pose_out *po;
    return results_layout(F, MM, &g, &nw, &cn, &mk, &po).bytes();
}
void layout_results(fid_ctx *c, int F)
{
    const int MM = c->lim.max_markers_per_frame;
    unsigned *h_nwork;  // (the work counters have no host twin)
    const MemLayout d = results_layout(F, MM, &c->d_global, &c->d_nwork, &c->d_counts, &c->d_markers, &c->d_poses, &c->res_clear_bytes, &c->res_markers_end);
    d.bind(c->d_res);
    results_layout(F, MM, &c->h_global, &h_nwork, &c->h_counts, &c->h_markers, &c->h_poses).bind(c->h_res);
    c->res_poses_off = c->res_markers_end;
    c->res_poses_end = d.bytes();
}

template <int NW, bool SPLIT>
void launch_thr_stream(dim3 grid, hipStream_t st, const uint8_t *g, long long gfstride, uint32_t *masks, const DevParams &P, int RS, int xcd_map)
{
    using S = ThrStream<3, 4, 13, NW>;
    fid_launch_log("k_threshold_stream", S::NT, S::LDS_BYTES);
    k_threshold_stream<3, 4, 13, NW, SPLIT><<<grid, dim3(S::NT), S::LDS_BYTES, st>>>(g, gfstride, masks, P, RS, xcd_map);
}

fid_status apply_params(fid_ctx *c, const fid_params *p)
{
    if (p->adaptiveThreshWinSizeMin < 3 || p->adaptiveThreshWinSizeMax < p->adaptiveThreshWinSizeMin ||
        p->adaptiveThreshWinSizeStep <= 0)
        return FID_E_INVALID_ARG;
    if (!(p->minMarkerPerimeterRate > 0 && p->maxMarkerPerimeterRate > 0 && p->polygonalApproxAccuracyRate > 0 &&
          p->minCornerDistanceRate >= 0 && p->minDistanceToBorder >= 0 && p->minMarkerDistanceRate >= 0))
        return FID_E_INVALID_ARG;  // the CV_Assert set of _findMarkerContours / _filterTooCloseCandidates
    if (p->markerBorderBits <= 0) return FID_E_INVALID_ARG;
    int nsc = (p->adaptiveThreshWinSizeMax - p->adaptiveThreshWinSizeMin) / p->adaptiveThreshWinSizeStep + 1;
    if (nsc > FID_MAX_SCALES) return FID_E_UNSUPPORTED;
    DevParams &P = c->P;
    P.nscales = nsc;
    P.rmax = 0;
    for (int i = 0; i < nsc; i++) {
        long long w = p->adaptiveThreshWinSizeMin + (long long)i * p->adaptiveThreshWinSizeStep;
        if (w % 2 == 0) w++;
        if (w > FID_MAX_THR_WIN) {
            c->last_error = "adaptive threshold window " + std::to_string(w) + " px: windows above " + std::to_string(FID_MAX_THR_WIN) +
                            " px (2 x 8191 + 1) are not supported";
            return FID_E_UNSUPPORTED;
        }
        P.win[i] = (int)w;
        if (w / 2 > P.rmax) P.rmax = (int)(w / 2);
    }
    // (rmax <= 40: k_threshold; above, k_threshold_wide -- any window up to FID_MAX_THR_WIN)
    {
        // adaptiveThreshold: idelta = type == THRESH_BINARY ? cvCeil(delta) : cvFloor(delta); aruco passes THRESH_BINARY_INV
        double cdelta = p->adaptiveThreshConstant;
        int i = (int)cdelta;
        P.idelta = i - (i > cdelta);  // cvFloor
    }
    P.polyAcc = p->polygonalApproxAccuracyRate;
    P.minCornerDistRate = p->minCornerDistanceRate;
    P.minMarkerDistRate = p->minMarkerDistanceRate;
    P.minDistToBorder = p->minDistanceToBorder;
    P.markerSize = c->dict_ms;
    P.borderBits = p->markerBorderBits;
    P.cellSize = p->perspectiveRemovePixelPerCell;
    P.cellMargin = (int)(p->perspectiveRemoveIgnoredMarginPerCell * p->perspectiveRemovePixelPerCell);
    if (P.markerSize + 2 * P.borderBits > FID_MAX_CELLS) {
        c->last_error = "markerSize + 2 x markerBorderBits = " + std::to_string(P.markerSize + 2 * P.borderBits) + " cells: at most " +
                        std::to_string(FID_MAX_CELLS) + " are supported";
        return FID_E_UNSUPPORTED;
    }
    if (P.cellSize < 1 || P.cellSize - 2 * P.cellMargin < 1) return FID_E_UNSUPPORTED;
    if ((long long)(P.markerSize + 2 * P.borderBits) * P.cellSize > FID_MAX_PATCH) {
        c->last_error = "unwarped patch of (markerSize + 2 x markerBorderBits) x perspectiveRemovePixelPerCell = " +
                        std::to_string((long long)(P.markerSize + 2 * P.borderBits) * P.cellSize) + " px a side: at most " +
                        std::to_string(FID_MAX_PATCH) + " are supported";
        return FID_E_UNSUPPORTED;
    }
    P.minOtsuStdDev = p->minOtsuStdDev;
    P.maxBorderErr = (int)(c->dict_ms * c->dict_ms * p->maxErroneousBitsInBorderRate);
    P.maxCorr = (int)((double)c->dict_maxc * p->errorCorrectionRate);
    P.nMarkers = c->dict_n;
    P.nbytes = (c->dict_ms * c->dict_ms + 7) / 8;
    // 0 CORNER_REFINE_NONE, 1 CORNER_REFINE_SUBPIX, 2 CORNER_REFINE_CONTOUR (the node reaches all three: aruco_detect.cpp:274-283,
    // 700-711).  3 = CORNER_REFINE_APRILTAG replaces the whole candidate search and is not something the node can select.
    if (p->cornerRefinementMethod < 0 || p->cornerRefinementMethod > 2) return FID_E_UNSUPPORTED;
    P.refine = p->cornerRefinementMethod;
    P.subpixWin = p->cornerRefinementWinSize;
    if (P.refine == 1 && (P.subpixWin < 1 || P.subpixWin > SP_MAXWIN_MAX || p->cornerRefinementMaxIterations < 1 ||
                     !(p->cornerRefinementMinAccuracy > 0))) {
        if (P.subpixWin > SP_MAXWIN_MAX)
            c->last_error = "cornerRefinementWinSize " + std::to_string(P.subpixWin) + ": at most " + std::to_string(SP_MAXWIN_MAX) +
                            " is supported with CORNER_REFINE_SUBPIX";
        return FID_E_INVALID_ARG;
    }
    {
        int mi = p->cornerRefinementMaxIterations;
        P.subpixMaxIter = mi < 1 ? 1 : (mi > 100 ? 100 : mi);
        double e = p->cornerRefinementMinAccuracy > 0 ? p->cornerRefinementMinAccuracy : 0.;
        P.subpixEps = e * e;
    }
    c->params = *p;
    // cornerSubPix weight mask, computed once on the host exactly as cornersubpix.cpp does (float expf)
    if (P.refine == 1) {
        int win = P.subpixWin, ww = 2 * win + 1;
        std::vector<float> mask((size_t)ww * ww);
        for (int i = 0; i < ww; i++) {
            float y = (float)(i - win) / win;
            float vy = expf(-y * y);
            for (int j = 0; j < ww; j++) {
                float x = (float)(j - win) / win;
                mask[(size_t)i * ww + j] = (float)(vy * expf(-x * x));
            }
        }
        HIPCHK(c, hipMemcpy(c->d_subpix_mask, mask.data(), mask.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return FID_OK;
}

void set_geometry(fid_ctx *c, int W, int H, int gstride, int F)
{
    DevParams &P = c->P;
    P.W = W;
    P.H = H;
    P.gstride = gstride;
    P.WW = (W + 31) / 32;
    P.TC = MASK_PADW + roundup(W, 128) / 32 + 1;  // one zero tile column left and right (threshold tiles are 128 px wide)
    P.TR = (H + 2 + MT_ROWS - 1) / MT_ROWS + 1;  // + one zero tile row: a 2 x 2 tile window always exists
    P.nframes = F;
    int maxdim = W > H ? W : H;
    P.minPerim = (int)(unsigned int)(c->params.minMarkerPerimeterRate * maxdim);
    P.maxPerim = (int)(unsigned int)(c->params.maxMarkerPerimeterRate * maxdim);
    P.maxStarts = c->lim.max_starts_per_frame;
    P.maxContours = c->lim.max_contours_per_frame;
    P.maxCands = c->lim.max_candidates_per_frame;
    P.maxMarkers = c->lim.max_markers_per_frame;
    P.maxChunks = c->max_chunks;
    // tracing seeds: the denser the grid, the shorter the longest seed-free stretch (the latency of a single frame) and the
    // more segments (tables, link / chain work).  Small calls take the densest grid their tables have room for.
    {
        int sh = 4;  // 128 px: batches (measured on the 256-frame bench batch: 64 px and 256 px are both slower)
        if (F <= 16 && P.maxContours >= 32768 && c->max_chunks >= 2 * 65536) sh = 3;  // 64 px
        if (F <= 2 && P.maxContours >= 65536 && c->max_chunks >= 4 * 65536) sh = 2;    // 32 px (one frame: 0.98 ms against 1.00 at 64 px)
        if (c->tune.seed_shift > 0) sh = c->tune.seed_shift;
        P.seedShift = sh < SEED_SHIFT_MIN ? SEED_SHIFT_MIN : (sh > SEED_SHIFT_MAX ? SEED_SHIFT_MAX : sh);
        P.seedHashCap = c->seed_hash_cap;
    }
}

size_t masks_elems(const fid_ctx *c, int W, int H, int F)
{
    int TC = MASK_PADW + roundup(W, 128) / 32 + 1, TR = (H + 2 + MT_ROWS - 1) / MT_ROWS + 1;
    return (size_t)F * c->P.nscales * TR * TC * MT_ROWS;
}

// the streams of sub-batches 0 .. nsub - 1 (and their auxiliary streams under cycle tracing), made on first use
fid_status ensure_streams(fid_ctx *c, int nsub, int F)
{
    if (c->piece_chain) nsub = 2;  // (piece k works on main stream k & 1 and auxiliary stream k & 1)
    for (int sb = 0; sb < nsub && sb < fid_ctx::MAX_SUB; sb++) {
        // (sub-batch 0 runs on the context's own stream, which has nothing else to do while a call is under way: a resident batch
        //  then works on four streams -- two sub-batches, two auxiliary -- which is what the HIP runtime's DEFAULT of four hardware
        //  queues carries side by side; with a fifth and sixth stream alive the default cost 17 % against GPU_MAX_HW_QUEUES >= 8)
        if (sb == 0) c->sub_stream[0] = c->stream;
        else if (!c->sub_stream[sb] && nsub > 1) HIPCHK(c, hipStreamCreateWithPriority(&c->sub_stream[sb], hipStreamNonBlocking, c->sub_prio[sb]));
        if (!c->aux_stream[sb] && !c->whole_border_walk) HIPCHK(c, hipStreamCreateWithPriority(&c->aux_stream[sb], hipStreamNonBlocking, c->sub_prio[sb]));
    }
    // one piece = two streams so far: a third one still fits the runtime's default of four hardware queues
    // (only for calls of a few frames -- the node's shape: a 256-frame batch of a chain is one piece too, but two contexts in turn
    //  would then hold six streams, and more than four live streams cost the batch 17 % in round 3)
    if (nsub == 1 && F <= 16 && !c->whole_border_walk && !c->idx_stream && c->tune.idx_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->idx_stream, hipStreamNonBlocking));
    return FID_OK;
}

// how a call of F frames is cut into sub-batches (run_detect; fid_detect_batch sends the frames up in the same pieces):
// sub-batch sb = frames [f0[sb], f0[sb + 1])
struct SubPlan {
    int nsub;
    int f0[fid_ctx::MAX_SUB + 1];
};
SubPlan plan_sub_batches(const fid_ctx *c, int F)
{
    const fid_ctx::Tuning &t = c->tune;
    SubPlan pl;
    if (c->chained && t.sub_frames <= 0 && !t.sub_shares_set) {
        // a batch in a chain of batches on two contexts (fid_order_after) IS the other half: the batch before it on the other
        // context plays the part of the first sub-batch, for ever, with no call boundary at which the last piece's latency-bound
        // end has the chip to itself.  Measured, 256 frames a batch, two contexts: whole batches 30.5 k frames/s, 64 % + 36 %
        // pieces 29.5 k (and 26.5 k for one context, one call after the other).
        pl.nsub = 1;
        pl.f0[0] = 0;
        pl.f0[1] = F;
        return pl;
    }
    if (t.sub_frames <= 0 && c->host_feed && F >= 64) {
        // frames that come up from the host while the call runs (the link, ~45 GB/s under load, is slower than the kernels):
        // four pieces -- the first kernels start after a fifth of the copy, the copy engine never idles, and what is left to
        // compute when the last byte has landed is a small piece.  The rate is insensitive to the split: the step is the arrival
        // of the first piece plus the kernels' time at the lower efficiency of small sub-batches
        pl.nsub = 4;
        int acc = 0;
        for (int k = 0; k < 4; k++) {
            pl.f0[k] = acc;
            acc += k == 3 ? F - acc : (F * t.feed_share[k] + 50) / 100;
        }
        pl.f0[4] = F;
        return pl;
    }
    if (c->piece_chain) {
        pl.nsub = t.pieces < fid_ctx::MAX_SUB ? t.pieces : fid_ctx::MAX_SUB;
        for (int k = 0; k <= pl.nsub; k++) pl.f0[k] = (int)((long long)F * k / pl.nsub);
        return pl;
    }
    // resident frames: two halves measured best (more streams fight for CUs)
    int per = t.sub_frames > 0 ? t.sub_frames : (F >= 32 ? (F + 1) / 2 : F);
    int nsub = (F + per - 1) / per;
    if (nsub > fid_ctx::MAX_SUB) {
        nsub = fid_ctx::MAX_SUB;
        per = (F + nsub - 1) / nsub;
        nsub = (F + per - 1) / per;
    }
    pl.nsub = nsub;
    for (int k = 0; k <= nsub; k++) pl.f0[k] = k * per < F ? k * per : F;
    if (t.sub_frames <= 0 && F >= 32) {
        // the sub-batches do not run in step: the first one's kernels meet less of the others' (its find_starts runs beside a
        // threshold, the second one's beside a seed walk and the probes), so with equal pieces it is through ~2 ms earlier and
        // the last one's latency-bound tail has the chip to itself.  Decreasing pieces even that out (FID_SUB_SHARES, per cent).
        const int n = t.n_sub_share, *sh = t.sub_share;
        int sum = 0;
        for (int k = 0; k < n; k++) sum += sh[k];
        if (n >= 1 && sum > 0) {
            pl.nsub = n;
            int acc = 0;
            for (int k = 0; k < n; k++) {
                pl.f0[k] = (int)((long long)F * acc / sum);
                acc += sh[k];
            }
            pl.f0[n] = F;
            // (no empty piece)
            for (int k = 1; k <= n; k++)
                if (pl.f0[k] <= pl.f0[k - 1]) pl.f0[k] = pl.f0[k - 1] + 1 < F ? pl.f0[k - 1] + 1 : F;
            while (pl.nsub > 1 && pl.f0[pl.nsub - 1] >= F) pl.nsub--;
            pl.f0[pl.nsub] = F;
        }
    }
    return pl;
}

// The whole detection pipeline for F frames whose gray images are resident at d_gray, in two halves: enqueue_detect puts every
// kernel and the result copies on the context's streams and returns (no host wait anywhere), finish_detect waits for them and
// hands the markers out.  fid_detect_device / fid_detect_batch call one after the other; fid_submit_device / fid_collect expose
// the halves, so that a caller with a stream of batches keeps two or three contexts in flight and the latency-bound tail of one
// batch runs under the front of the next.
// Everything a detect call can be refused for, checked BEFORE anything is put on a stream: feed_and_enqueue queues host -> device
// copies of the caller's buffer in front of the kernels, and a call that is then refused must not leave DMA from that buffer in
// flight (the caller may free it as soon as it sees the error).
// bytes one pixel occupies in a row; 0 = not an encoding this library takes.  FID_ENC_BIGENDIAN is only meaningful (and only
// accepted) on the 16-bit layouts.
static int enc_bytes_per_pixel(int enc)
{
    const int base = enc & 0xff;
    if (enc & ~(0xff | FID_ENC_BIGENDIAN)) return 0;
    if ((enc & FID_ENC_BIGENDIAN) && !(base >= FID_ENC_MONO16 && base <= FID_ENC_RGBA16)) return 0;
    switch (base) {
    case FID_ENC_MONO8: case FID_ENC_BAYER_RGGB8: case FID_ENC_BAYER_BGGR8: case FID_ENC_BAYER_GBRG8: case FID_ENC_BAYER_GRBG8: return 1;
    case FID_ENC_BGR8: case FID_ENC_RGB8: return 3;
    case FID_ENC_BGRA8: case FID_ENC_RGBA8: return 4;
    case FID_ENC_MONO16: case FID_ENC_YUV422: return 2;
    case FID_ENC_BGR16: case FID_ENC_RGB16: return 6;
    case FID_ENC_BGRA16: case FID_ENC_RGBA16: return 8;
    default: return 0;
    }
}

fid_status check_call(fid_ctx *c, int F, int W, int H, int stride, fid_encoding enc)
{
    if (F < 1 || F > c->lim.max_batch || W < 8 || H < 8 || W > c->lim.max_width || H > c->lim.max_height || W > 8191 || H > 8191)  // 13-bit checkpoint packing
        return FID_E_INVALID_ARG;
    const int bpp = enc_bytes_per_pixel(enc);
    if (bpp == 0 || stride < W * bpp) return FID_E_INVALID_ARG;
    if ((enc & 0xff) == FID_ENC_YUV422 && (W & 1)) return FID_E_INVALID_ARG;  // (a UYVY row is whole pixel pairs)
    const int maxdim = W > H ? W : H;
    if ((unsigned)(c->params.maxMarkerPerimeterRate * maxdim) > 36000u) return FID_E_UNSUPPORTED;  // contour points live in LDS
    const size_t pitch = (size_t)((int)(unsigned)(c->params.maxMarkerPerimeterRate * maxdim) / CK + 3);  // chunk_tab_pitch
    if ((size_t)F * 2 * c->lim.max_contours_per_frame * pitch > c->ckpts_elems) {
        c->last_error = "chunk table too small for this image size / maxMarkerPerimeterRate";
        return FID_E_UNSUPPORTED;
    }
    return FID_OK;
}

// k_pose (+ k_pose_cov) on a stream.  Defined BEHIND enqueue_detect: the device code is emitted in the order in which the host code
// first names the kernels, and the counter files under profiles/ are keyed to its bytes.  For the same reason the stage functions
// below stand in the order front, whole-border, cycle tracing, tail, and name their kernels in the order the launch sequence always had
void pose_launch(fid_ctx *c, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, const fid_marker *d_markers, const int *d_n, int n_stride_ints,
                 const double *d_lens, int F, int per_frame, const PoseAsk &a, fid_pose_out *d_out, fid_pose_cov *d_cov);

// ---- Sub-batch `sb` of a call: frames [f0, f0 + Fs) of it, the streams they run on under the call's layout, and THEIR part of every
// per-frame buffer.  The buffers are the arrays of the HBM layout at the top of fid_device.h, every one indexed [frame][...]: "frames
// [f0, f0 + Fs) of buffer X" is X + f0 * (X's elements per frame), and that arithmetic stands here and nowhere else -- the kernels
// get these pointers with DevParams::nframes = Fs and index them from frame 0.
struct SubBatch {
    int sb, nsub, f0, Fs;
    DevParams P;  // the call's, with nframes = Fs
    // main stream; auxiliary stream (cycle tracing: the seedless chain; the piece chain: the candidate tail as well); the stream of
    // k_seed_index (a stream of its own for a call of ONE piece of up to 16 frames, else the auxiliary one); the stream of the tail
    hipStream_t st, sa, si, tail;
    hipEvent_t *ev;  // its row of fid_ctx::sub_ev
    const uint8_t *src;  // the caller's frames: colour input, k_to_gray reads them and writes gray_dst
    uint8_t *gray_dst;
    const uint8_t *g;  // the gray frames the detector sees (mono8 input: the caller's, in place), gfstride bytes apart
    long long gfstride;
    uint32_t *masks, *tab, *pool;  // (chunk table: rows of the seeds, then of the survivors; chain codes: CKW words per chunk of CK points)
    uint2 *starts, *surv1, *surv;
    uint4 *contours;
    DevCounts *counts;
    // cycle tracing (nullptr in a context created for the whole-border walk)
    uint2 *seedq;
    DevSegC *segs;
    DevPend *pend;
    unsigned long long *seedhash;
    uint4 *wres, *cinfo, *recs;
    uint32_t *cbase, *dense;  // (dense: one code byte per point)
    // the candidate tail
    DevCand *cands, *sorted, *filtered;
    float4 *cmeta;
    uint32_t *nearb;
    unsigned *worklist, *nwork;
    DevIdent *ident;
    uint8_t *bits;
    fid_marker *pre, *markers, *filter_scratch;
    int *accsrc, *mksrc;
    fid_pose_out *poses;
    fid_pose_cov *pcov;  // (nullptr until the first _cov call)
};

template <typename T>
inline T *frames_from(T *base, int f0, size_t per_frame)
{
    return base ? base + (size_t)f0 * per_frame : nullptr;
}

SubBatch sub_batch_view(fid_ctx *c, const SubPlan &plan, int sb, const uint8_t *d_src, long long fstride, const uint8_t *gray, long long gfstride, int W,
                        int H)
{
    SubBatch s;
    s.sb = sb;
    s.nsub = plan.nsub;
    s.f0 = plan.f0[sb];
    s.Fs = plan.f0[sb + 1] - s.f0;
    s.P = c->P;
    s.P.nframes = s.Fs;
    const DevParams &P = s.P;
    const int f0 = s.f0, lane = c->piece_chain ? (sb & 1) : sb;  // (piece k of a chain works on main stream k & 1 and auxiliary stream k & 1)
    s.st = s.nsub > 1 ? c->sub_stream[lane] : c->stream;
    s.sa = c->aux_stream[lane];
    s.si = (s.nsub == 1 && s.Fs <= 16 && c->idx_stream) ? c->idx_stream : s.sa;
    s.tail = c->piece_chain ? s.sa : s.st;
    s.ev = c->sub_ev[sb];
    const size_t MC = (size_t)P.maxCands, MM = (size_t)P.maxMarkers, MCn = (size_t)P.maxContours, msb = (size_t)(P.markerSize + 2 * P.borderBits);
    s.src = d_src + (long long)f0 * fstride;
    s.gray_dst = c->d_gray + (size_t)f0 * W * H;
    s.g = gray + (long long)f0 * gfstride;
    s.gfstride = gfstride;
    const size_t MS = (size_t)P.maxStarts, chunks = (size_t)P.maxChunks;
    s.masks = frames_from(c->d_masks, f0, (size_t)P.nscales * P.TR * P.TC * MT_ROWS);
    s.starts = frames_from(c->d_starts, f0, MS), s.surv1 = frames_from(c->d_surv1, f0, MS), s.surv = frames_from(c->d_surv, f0, MS);
    s.contours = frames_from(c->d_contours, f0, MCn);
    s.tab = frames_from(c->d_ckpts, f0, 2 * MCn * chunk_tab_pitch(P)), s.pool = frames_from(c->d_pool, f0, chunks * CKW);
    s.counts = c->d_counts + f0;
    s.seedq = frames_from(c->d_seedq, f0, MCn), s.segs = frames_from(c->d_segs, f0, MCn), s.pend = frames_from(c->d_pend, f0, MCn);
    s.seedhash = frames_from(c->d_seedhash, f0, (size_t)P.seedHashCap);
    s.wres = frames_from(c->d_wres, f0, MCn), s.cinfo = frames_from(c->d_cinfo, f0, MCn), s.recs = frames_from(c->d_recs, f0, 2 * MCn);
    s.cbase = frames_from(c->d_cbase, f0, MCn), s.dense = frames_from(c->d_dense, f0, chunks * (CK / 4));
    s.cands = frames_from(c->d_cands, f0, MC), s.sorted = frames_from(c->d_sorted, f0, MC), s.filtered = frames_from(c->d_filtered, f0, MC);
    s.cmeta = frames_from(c->d_cmeta, f0, MC), s.nearb = frames_from(c->d_near, f0, MC * (MC / 32));
    s.worklist = frames_from(c->d_worklist, f0, MC), s.nwork = c->d_nwork + sb;  // (one work-list counter per sub-batch)
    s.ident = frames_from(c->d_ident, f0, MC), s.bits = frames_from(c->d_bits, f0, MC * msb * msb);
    s.pre = frames_from(c->d_pre, f0, MM), s.markers = frames_from(c->d_markers, f0, MM), s.filter_scratch = frames_from(c->d_filter_scratch, f0, MC);
    s.accsrc = frames_from(c->d_accsrc, f0, MC), s.mksrc = frames_from(c->d_mksrc, f0, MM);
    s.poses = frames_from(c->d_poses, f0, MM), s.pcov = frames_from(c->pcov.data(), f0, MM);
    return s;
}

// ---- Launch geometry of a sub-batch: every workgroup count and dynamic-LDS size of the chain, from the tunables, the parameters and
// the sub-batch's frame count.  The kernels with a fixed number of workgroups per frame are sized for batches; what a smaller call
// gets instead is decided by its regime, once:
//   ONE_OR_TWO  Fs <= 2: every seed in flight at once (256-workgroup walker cap, a lane for every seed in k_seg_cycles<48>)
//   FEW         Fs < 16: more workgroups per frame (gm = 16 / Fs of them for each one of a batch -- 1 again from 9 frames on)
//   BATCH       Fs >= 16
// (the index stream of a call of one piece is a matter of streams, not of grids: SubBatch::si, up to 16 frames)
struct Grids {
    enum Regime { ONE_OR_TWO, FEW, BATCH } regime;
    int gm;
    // the front
    enum Threshold { THR_STREAM, THR_WIDE, THR_TILES } thr;  // the node's window table / windows above 81 px / any other table
    dim3 thr_grid;
    int thr_rows;  // rows per workgroup (k_threshold_stream: RS; k_threshold_wide: BH)
    size_t thr_lds;
    unsigned k2blocks;
    bool split_seeds;
    int seed_blocks;
    // the contour stages
    int wb, wb3, swb, cpb, scb;
    bool single_pass;
    int cap1;
    size_t lds1, lds2;
    // the candidate tail
    int sort_y, light_blocks;
    size_t resolve_lds;
    int near_words;
    int ident_blocks, subpix_blocks;
    size_t ident_lds, filter_lds;
};

Grids launch_grids(const fid_ctx::Tuning &t, const DevParams &P, int Fs)
{
    Grids G;
    const int W = P.W, H = P.H;
    G.regime = Fs <= 2 ? Grids::ONE_OR_TWO : (Fs < 16 ? Grids::FEW : Grids::BATCH);
    // kernels with a fixed number of workgroups per frame (sized for batches): a call of a few frames gets more of them
    const int gm = G.gm = G.regime == Grids::BATCH ? 1 : 16 / Fs;
    // ---- K1
    bool node_table = P.nscales == 13;  // 3, 7, ..., 51: the node defaults (aruco_detect.cpp:690-693)
    for (int i = 0; i < P.nscales && node_table; i++) node_table = P.win[i] == 3 + 4 * i;
    G.thr_lds = 0;
    if (node_table) {
        // strips of 64 * NW columns, cut into row segments so that the grid fills the chip (a segment pays a warm-up
        // of about ten steps, so they are kept as tall as the batch allows)
        const int cols = 64 * t.thr_nw, strips = (W + cols - 1) / cols;
        int RS = t.thr_rows;
        if (RS <= 0) {
            int segs = (1536 + strips * Fs - 1) / (strips * Fs);
            const int maxsegs = (H + 63) / 64;
            segs = segs < 1 ? 1 : (segs > maxsegs ? maxsegs : segs);
            RS = (H + segs - 1) / segs;
        }
        RS = (RS + 3) & ~3;
        G.thr = Grids::THR_STREAM;
        G.thr_grid = dim3(strips, (H + RS - 1) / RS, Fs);
        G.thr_rows = RS;
    } else if (P.rmax > 40) {
        // windows above 81 px: bands of whole rows, enough of them to fill the chip (a band pays a closed-form start of its
        // running column sums, up to min(2 rmax + 1, H) rows per scale, so they are not cut below 16 rows)
        int bands = (512 + Fs - 1) / Fs;
        const int maxb = (H + 15) / 16;
        bands = bands < 1 ? 1 : (bands > maxb ? maxb : bands);
        const int BH = (H + bands - 1) / bands;
        G.thr = Grids::THR_WIDE;
        G.thr_grid = dim3((H + BH - 1) / BH, 1, Fs);
        G.thr_rows = BH;
        G.thr_lds = (size_t)(W + 1 + THRW_NT / 64) * sizeof(unsigned long long);
    } else {
        int R = P.rmax, RW = TX + 2 * R, RH = TY + 2 * R, PT = (RW + 1) | 1;
        G.thr = Grids::THR_TILES;
        G.thr_grid = dim3((W + TX - 1) / TX, (H + TY - 1) / TY, Fs);
        G.thr_rows = 0;
        G.thr_lds = (size_t)(RH + 1) * PT * sizeof(uint32_t);
    }
    // ---- K2
    // the tracing seeds: on the 128 px grid of batches few word columns and rows hold any, and a kernel of their own finds them
    // (split); on the denser grids of small calls every word column or every second one is a grid column: k_find_starts<true>
    G.split_seeds = t.seed_kernel ? t.seed_kernel == 1 : P.seedShift >= 4;
    {
        long long groups = (long long)P.nscales * P.TR * ((P.WW + 15) / 16);  // two groups per wave and iteration
        long long k2blocks = (groups + 7) / 8;
        if (k2blocks > 256) k2blocks = 256;
        G.k2blocks = (unsigned)k2blocks;
    }
    G.seed_blocks = 0;
    if (G.split_seeds) {
        const SeedUnits su = seed_units(P);
        // (a wave per unit: a batch gives a frame 32 workgroups, a call of a few frames a workgroup for every four units)
        const int smax = G.regime == Grids::BATCH ? 32 : 512;
        G.seed_blocks = (su.n + 3) / 4 < smax ? (su.n + 3) / 4 : smax;
    }
    // ---- K3, K4
    // persistent walker workgroups (WALK_WAVES waves each) per frame: about 16 waves per CU over the sub-batch
    int wb = t.walk_blocks > 0 ? t.walk_blocks : (3072 / WALK_WAVES + Fs - 1) / Fs;  // (measured: 6 per frame at 128 frames beats 8 and 12)
    // (the walks of one frame want every seed in flight at once: one frame, 32 px grid: seed walk 0.25 -> 0.115 ms)
    const int wcap = t.walk_blocks_cap > 0 ? t.walk_blocks_cap : (G.regime == Grids::ONE_OR_TWO ? 256 : 64);
    G.wb = wb = wb < 2 ? 2 : (wb > wcap ? wcap : wb);
    const int wb2 = wb > 1 ? wb / 2 : 1;  // the two walks share the CUs' LDS
    G.wb3 = t.walk2_div > 0 ? (wb / t.walk2_div > 0 ? wb / t.walk2_div : 1) : wb2;
    // about 4 walker waves per CU over the sub-batch (34 KB LDS per 2-wave workgroup: two of them leave a CU room for
    // the other sub-batch's kernels; 8 waves per CU measured 7 % slower end to end)
    int swb = t.sw_blocks > 0 ? t.sw_blocks : (1024 / SW_WAVES + Fs - 1) / Fs;
    G.swb = swb < 2 ? 2 : (swb > 4 * wcap ? 4 * wcap : swb);
    G.cpb = t.copy_blocks > 0 ? t.copy_blocks : 256;
    // (batches: one pass over every start; 16 waves a frame that keep their lanes filled -- a call of a few frames wants every start
    //  in flight at once, in two passes)
    G.single_pass = t.probe_passes == 1 && t.probe_refill && gm == 1;
    // (a call of one or two frames: a lane for every seed at once -- a workgroup that came round to a second 64 seeds walked a
    //  second longest cycle behind the first, 2 x 26 us of the single frame's 55 us)
    G.scb = G.regime == Grids::ONE_OR_TWO ? (int)((P.maxContours + 63) / 64 < 4096 ? (P.maxContours + 63) / 64 : 4096) : 32 * gm * t.light_x;
    // approxPolyDP: short contours with a small LDS footprint first, then the long / flagged ones
    G.cap1 = pts_cap_first(P);
    G.lds1 = k_approx_lds_bytes(G.cap1);
    G.lds2 = k_approx_lds_bytes(P.maxPerim + 1);
    // ---- K5 .. K7
    const size_t MC = (size_t)P.maxCands;
    // (a rank sort: every candidate is compared with all of them -- a call of a few frames gives the frame sixteen workgroups)
    G.sort_y = (t.light_x > 1 || G.regime != Grids::BATCH) ? 16 : 1;
    G.light_blocks = 32 * gm * t.light_x;
    // k_resolve: sizes, labels, component sizes; the rest holds the near triangle (64 KB: fits beside two seed-walker workgroups of
    // the other sub-batch on a CU; with 96 KB the kernel waited for whole CUs to drain)
    G.resolve_lds = (size_t)t.resolve_lds_kb * 1024;
    G.near_words = t.resolve_serial ? 0 : (int)((G.resolve_lds - 3 * MC * 4) / 4);
    const int SZ = (P.markerSize + 2 * P.borderBits) * P.cellSize;
    G.ident_blocks = t.tail_grid > 0 ? t.tail_grid : 256 * 4;
    G.ident_lds = (size_t)SZ * SZ;
    G.filter_lds = (size_t)t.filter_lds * sizeof(fid_marker);
    {
        long long items = (long long)Fs * P.maxMarkers * 4;
        const long long bcap = t.tail_grid > 0 ? 4LL * t.tail_grid : 256 * 16;
        G.subpix_blocks = (int)(items < bcap ? items : bcap);
    }
    return G;
}

// a stage boundary of the sub-batch (FID_PROFILE)
inline void mark(const fid_ctx *c, const SubBatch &s, hipStream_t st, int idx)
{
    if (c->profile) (void)hipEventRecord(s.ev[idx], st);
}
// a point at which the next batch of a chain (fid_order_after, on another context) may start: tail_ev is recorded at the first one
// the LAST sub-batch passes at or behind Tuning::chain_at (a point the mode in use does not pass falls through to the next one that it does)
inline void chain_point(fid_ctx *c, const SubBatch &s, hipStream_t st, int pt)
{
    if (s.sb == s.nsub - 1 && !c->tail_recorded && !c->blocking && c->tune.chain_at <= pt) {  // (an event record costs the stream ~6 us)
        (void)hipEventRecord(c->tail_ev, st);
        c->tail_recorded = true;
    }
}

// ---- The front, on the main stream: gray conversion, threshold, and under cycle tracing the start / seed search -- every
// sub-batch's find_starts is then queued before any walk, and (fs_barrier) the walks of all sub-batches wait for the last find_starts:
// beside another sub-batch's seed walk and probes a find_starts took 2.5 ms for 92 frames, beside another find_starts 1.1 ms for 164.
// Records fs_done; chain point 0.
fid_status stage_front(fid_ctx *c, const SubBatch &s, const Grids &G, const fid_ctx::Pending &in)
{
    const DevParams &P = s.P;
    const fid_ctx::Tuning &t = c->tune;
    hipStream_t st = s.st;
    const int Fs = s.Fs;
    mark(c, s, st, 0);
    // ---- K0: mono8 device input is used in place (any stride); colour goes through k_to_gray
    if (in.enc != FID_ENC_MONO8 && (int)in.enc <= FID_ENC_RGBA8)
        hipLaunchKernelGGL(k_to_gray, dim3(2048), dim3(256), 0, st, s.src, in.stride, in.fstride, (int)in.enc, s.gray_dst, P.W, P.H, Fs);
    else if (in.enc != FID_ENC_MONO8)  // (ABI 7: Bayer mosaics, 16-bit layouts, UYVY -- cv_bridge's conversion and BGR2GRAY in one pass)
        hipLaunchKernelGGL(k_raw_to_gray, dim3((P.W + 255) / 256, (P.H + 3) / 4, Fs), dim3(64, 4), 0, st, s.src, in.stride, in.fstride, (int)in.enc,
                           s.gray_dst, P.W, P.H);
    mark(c, s, st, ST_GRAY + 1);
    // ---- K1
    if (G.thr == Grids::THR_STREAM) {
        if (t.thr_nw == 5 && t.thr_split) launch_thr_stream<5, true>(G.thr_grid, st, s.g, s.gfstride, s.masks, P, G.thr_rows, t.thr_xcd);
        else if (t.thr_nw == 5) launch_thr_stream<5, false>(G.thr_grid, st, s.g, s.gfstride, s.masks, P, G.thr_rows, t.thr_xcd);
        else if (t.thr_split) launch_thr_stream<3, true>(G.thr_grid, st, s.g, s.gfstride, s.masks, P, G.thr_rows, t.thr_xcd);
        else launch_thr_stream<3, false>(G.thr_grid, st, s.g, s.gfstride, s.masks, P, G.thr_rows, t.thr_xcd);
    } else if (G.thr == Grids::THR_WIDE) {
        fid_launch_log("k_threshold_wide", THRW_NT, G.thr_lds);
        hipLaunchKernelGGL((k_threshold_wide<THRW_NT, THRW_WT>), G.thr_grid, dim3(THRW_NT), G.thr_lds, st, s.g, s.gfstride, s.masks, P, G.thr_rows);
    } else {
        hipLaunchKernelGGL((k_threshold<TX, TY, NT>), G.thr_grid, dim3(NT), G.thr_lds, st, s.g, s.gfstride, s.masks, P);
    }
    mark(c, s, st, ST_THRESH + 1);
    if (c->whole_border_walk) return FID_OK;  // (its start search heads the whole-border stage)
    // ---- K2
    if (G.split_seeds) {
        // the seeds come from a kernel of their own that only visits the grid lines (k_find_seeds), directly behind the
        // start search on the same stream.  (On the sub-batch's auxiliary stream, beside k_find_starts<false> and joined
        // in front of the seed walk by two events, it measured 0.2 - 0.5 % slower: profiles/r10_seed_split_ab.txt.)
        hipLaunchKernelGGL(k_find_starts<false>, dim3(G.k2blocks, Fs), dim3(256), 0, st, s.masks, s.starts, s.counts, c->d_global, (uint2 *)nullptr, P);
        mark(c, s, st, ST_STARTS + 1);
        hipLaunchKernelGGL(k_find_seeds, dim3(G.seed_blocks, Fs), dim3(256), 0, st, s.masks, s.counts, c->d_global, s.seedq, P);
    } else {
        hipLaunchKernelGGL(k_find_starts<true>, dim3(G.k2blocks, Fs), dim3(256), 0, st, s.masks, s.starts, s.counts, c->d_global, s.seedq, P);
        mark(c, s, st, ST_STARTS + 1);
    }
    if (s.nsub > 1) HIPCHK(c, hipEventRecord(c->fs_done[s.sb], st));
    chain_point(c, s, st, 0);
    return FID_OK;
}

// ---- The whole-border contour stage, all on the main stream: start search, two probe passes that sieve the starts, the walk of
// the survivors to the end, approxPolyDP
fid_status stage_whole_border(fid_ctx *c, const SubBatch &s, const Grids &G)
{
    const DevParams &P = s.P;
    hipStream_t st = s.st;
    const int Fs = s.Fs, gm = G.gm;
    hipLaunchKernelGGL(k_find_starts<false>, dim3(G.k2blocks, Fs), dim3(256), 0, st, s.masks, s.starts, s.counts, c->d_global, (uint2 *)nullptr, P);
    mark(c, s, st, ST_STARTS + 1);
    // ---- K3: sieve the starts twice, then walk the survivors to the end
    hipLaunchKernelGGL((k_probe<PROBE0_STEPS, 0>), dim3(64 * gm, Fs), dim3(256), 0, st, s.masks, s.starts, s.surv1, s.counts, c->d_global, P);
    hipLaunchKernelGGL((k_probe<PROBE1_STEPS, 1>), dim3(16 * gm, Fs), dim3(256), 0, st, s.masks, s.surv1, s.surv, s.counts, c->d_global, P);
    mark(c, s, st, ST_PROBE + 1);
    hipLaunchKernelGGL(k_walk_full<0>, dim3(G.wb, Fs), dim3(64 * WALK_WAVES), 0, st, s.masks, s.surv, s.contours, s.tab, s.pool, (DevSegC *)nullptr,
                       (DevPend *)nullptr, s.counts, c->d_global, P);
    mark(c, s, st, ST_WALK + 1);
    // ---- K4: short contours with a small LDS footprint first, then the long / flagged ones
    fid_launch_log("k_approx", 64, G.lds1);
    hipLaunchKernelGGL(k_approx, dim3(128 * gm, Fs), dim3(64), G.lds1, st, s.contours, s.tab, s.pool, s.cands, s.counts, P, G.cap1, 0,
                       (const uint32_t *)nullptr, (const uint32_t *)nullptr);
    fid_launch_log("k_approx", 64, G.lds2);
    hipLaunchKernelGGL(k_approx, dim3(16 * gm, Fs), dim3(64), G.lds2, st, s.contours, s.tab, s.pool, s.cands, s.counts, P, P.maxPerim + 1, 1,
                       (const uint32_t *)nullptr, (const uint32_t *)nullptr);
    mark(c, s, st, ST_APPROX + 1);
    return FID_OK;
}

// ---- The cycle-tracing contour stage (k_find_starts / k_find_seeds were queued by the front).  Main stream: the seeds walk their
// segments, link, the cycles become contour list A, copy, approxPolyDP.  Auxiliary stream, beside it: seed index, then the chain that
// only exists for borders WITHOUT a seed state (probe passes that drop a start at the first seed state, survivor walk, contour list B,
// copy, approxPolyDP) -- off the critical path, it used to be 2.9 ms of a 9.6 ms sub-batch.  Both append candidates; the streams join
// in front of the candidate tail (aux_join), or, in a chain of pieces, the tail goes on on the auxiliary stream (front_done).
//   main:       aux_fork . k_seed_walk [chain point 1] ................ (aux_idx) k_seg_link2 k_seg_cycles k_seg_copy [2] k_approx x 2 [3]
//   auxiliary:  (aux_fork) [k_seed_index aux_idx] probes k_walk_full<2> (aux_idx) k_seg_cycles k_seg_copy k_approx x 2 aux_join
//   index:      (aux_fork) k_seed_index aux_idx          -- a call of one piece of up to 16 frames; else on the auxiliary stream
fid_status stage_cycle_tracing(fid_ctx *c, const SubBatch &s, const Grids &G)
{
    const DevParams &P = s.P;
    const fid_ctx::Tuning &t = c->tune;
    hipStream_t st = s.st, sa = s.sa, si = s.si;
    const int Fs = s.Fs, gm = G.gm, sb = s.sb;
    const uint4 *probe_tables = (const uint4 *)c->d_probe_tables;
    HIPCHK(c, hipEventRecord(c->aux_fork[sb], st));
    HIPCHK(c, hipStreamWaitEvent(sa, c->aux_fork[sb], 0));
    // -- the main stream's first kernel goes out BEFORE the auxiliary chain's eight launches: the host needs ~15 us to
    //    enqueue those, and for a single frame the seed walk sat waiting behind them (round 4, cfg 2 timeline)
    mark(c, s, st, EV_SEEDWALK0);
    hipLaunchKernelGGL(k_seed_walk, dim3(G.swb, Fs), dim3(64 * SW_WAVES), 0, st, s.masks, s.seedq, s.tab, s.pool, s.segs, s.counts, c->d_global, P);
    mark(c, s, st, EV_SEEDWALK1);
    mark(c, s, st, ST_PROBE + 1);
    chain_point(c, s, st, 1);
    // -- auxiliary stream.  k_seed_index (the map seed state -> seed index, which only k_seg_link2 on the main stream and
    //    the auxiliary k_seg_cycles need) is off the auxiliary chain's critical path when the call is one piece: a stream of
    //    its own beside the probes (39 us of a single frame's 314 us contour stage)
    mark(c, s, sa, EV_SEEDLESS0);
    if (si != sa) HIPCHK(c, hipStreamWaitEvent(si, c->aux_fork[sb], 0));
    hipLaunchKernelGGL(k_seed_index, dim3(8 * gm, Fs), dim3(256), 0, si, s.seedq, s.seedhash, s.counts, P);
    HIPCHK(c, hipEventRecord(c->aux_idx[sb], si));
    if (G.single_pass) {  // (batches: one pass over every start)
        hipLaunchKernelGGL((k_probe_refill<PROBE1_STEPS, 2>), dim3(t.probe_single, Fs), dim3(256), 0, sa, s.masks, s.starts, s.surv, s.counts, c->d_global, P,
                           probe_tables);
    } else {
        if (t.probe_refill0 && gm == 1)
            hipLaunchKernelGGL((k_probe_refill<PROBE0_STEPS, 0>), dim3(t.probe_refill0, Fs), dim3(256), 0, sa, s.masks, s.starts, s.surv1, s.counts,
                               c->d_global, P, probe_tables);
        else
            hipLaunchKernelGGL((k_probe_lut<PROBE0_STEPS, 0>), dim3(64 * gm, Fs), dim3(256), 0, sa, s.masks, s.starts, s.surv1, s.counts, c->d_global, P,
                               probe_tables);
        if (t.probe_refill && gm == 1)  // (batches: 16 waves a frame that keep their lanes filled; a call of a few frames wants every start in flight at once)
            hipLaunchKernelGGL((k_probe_refill<PROBE1_STEPS, 1>), dim3(t.probe_refill, Fs), dim3(256), 0, sa, s.masks, s.surv1, s.surv, s.counts,
                               c->d_global, P, probe_tables);
        else
            hipLaunchKernelGGL((k_probe_lut<PROBE1_STEPS, 1>), dim3(16 * gm, Fs), dim3(256), 0, sa, s.masks, s.surv1, s.surv, s.counts, c->d_global, P,
                               probe_tables);
    }
    hipLaunchKernelGGL(k_walk_full<2>, dim3(G.wb3, Fs), dim3(64 * WALK_WAVES), 0, sa, s.masks, s.surv, s.wres, s.tab, s.pool, s.segs, s.pend, s.counts,
                       c->d_global, P);
    if (si != sa) HIPCHK(c, hipStreamWaitEvent(sa, c->aux_idx[sb], 0));  // (the survivors' seed look-ups need the map)
    hipLaunchKernelGGL(k_seg_cycles<0>, dim3(8 * gm, Fs), dim3(64), 0, sa, s.seedq, s.segs, s.pend, s.wres, s.contours, s.cinfo, s.cbase, s.recs,
                       s.counts, c->d_global, P, 1, 0);
    hipLaunchKernelGGL(k_seg_copy, dim3(G.cpb / 4 > 0 ? G.cpb / 4 : 1, Fs), dim3(256), 0, sa, s.recs, s.tab, s.pool, s.dense, s.counts, P, 1);
    fid_launch_log("k_approx", 64, G.lds1);
    hipLaunchKernelGGL(k_approx, dim3(32 * gm, Fs), dim3(64), G.lds1, sa, s.contours, s.tab, s.pool, s.cands, s.counts, P, G.cap1, 0, s.dense, s.cbase, 2);
    fid_launch_log("k_approx", 64, G.lds2);
    hipLaunchKernelGGL(k_approx, dim3(8 * gm, Fs), dim3(64), G.lds2, sa, s.contours, s.tab, s.pool, s.cands, s.counts, P, P.maxPerim + 1, 1, s.dense,
                       s.cbase, 2);
    mark(c, s, sa, EV_SEEDLESS1);
    HIPCHK(c, hipEventRecord(c->aux_join[sb], sa));
    // -- main stream, continued
    HIPCHK(c, hipStreamWaitEvent(st, c->aux_idx[sb], 0));
    hipLaunchKernelGGL(k_seg_link2, dim3(16 * gm, Fs), dim3(256), 0, st, s.seedq, s.segs, s.seedhash, s.counts, P);
    if (G.regime == Grids::ONE_OR_TWO)
        hipLaunchKernelGGL(k_seg_cycles<48>, dim3(G.scb, Fs), dim3(64), 0, st, s.seedq, s.segs, s.pend, s.wres, s.contours, s.cinfo, s.cbase, s.recs,
                           s.counts, c->d_global, P, 0, t.segc_warm);
    else
        hipLaunchKernelGGL(k_seg_cycles<0>, dim3(G.scb, Fs), dim3(64), 0, st, s.seedq, s.segs, s.pend, s.wres, s.contours, s.cinfo, s.cbase, s.recs,
                           s.counts, c->d_global, P, 0, 0);
    hipLaunchKernelGGL(k_seg_copy, dim3(G.cpb, Fs), dim3(256), 0, st, s.recs, s.tab, s.pool, s.dense, s.counts, P, 0);
    mark(c, s, st, ST_WALK + 1);
    chain_point(c, s, st, 2);
    fid_launch_log("k_approx", 64, G.lds1);
    hipLaunchKernelGGL(k_approx, dim3(128 * gm, Fs), dim3(64), G.lds1, st, s.contours, s.tab, s.pool, s.cands, s.counts, P, G.cap1, 0, s.dense, s.cbase, 1);
    fid_launch_log("k_approx", 64, G.lds2);
    hipLaunchKernelGGL(k_approx, dim3(16 * gm, Fs), dim3(64), G.lds2, st, s.contours, s.tab, s.pool, s.cands, s.counts, P, P.maxPerim + 1, 1, s.dense,
                       s.cbase, 1);
    mark(c, s, st, ST_APPROX + 1);
    chain_point(c, s, st, 3);
    if (c->piece_chain) {
        // the candidate tail of this piece moves to its auxiliary stream (behind the seedless chain, which is there already):
        // the main stream is free for the front of the piece after next
        HIPCHK(c, hipEventRecord(c->front_done[sb], st));
        HIPCHK(c, hipStreamWaitEvent(sa, c->front_done[sb], 0));
    } else {
        HIPCHK(c, hipStreamWaitEvent(st, c->aux_join[sb], 0));
    }
    return FID_OK;
}

// ---- The candidate tail, a chain of short latency-bound kernels on the sub-batch's tail stream: sort, near pairs, too-close
// filter, identification, marker filter, corner refinement, the remembered marker pose.  Records walk_done in front of it (staggered
// starts); chain points 4 (in front of the sort), 5 (behind the too-close filter) and the end
fid_status stage_tail(fid_ctx *c, const SubBatch &s, const Grids &G)
{
    const DevParams &P = s.P;
    const fid_ctx::Tuning &t = c->tune;
    hipStream_t st = s.tail;
    const int Fs = s.Fs;
    const size_t MC = (size_t)P.maxCands;
    if (s.nsub > 1 && t.stagger > 0) HIPCHK(c, hipEventRecord(c->walk_done[s.sb], st));
    chain_point(c, s, st, 4);
    // ---- K5
    fid_launch_log("k_sort_cands", 256, (size_t)(MC * 8));
    hipLaunchKernelGGL(k_sort_cands, dim3(Fs, G.sort_y), dim3(256), MC * 8, st, s.cands, s.sorted, s.cmeta, s.counts, P);
    mark(c, s, st, ST_SORT + 1);
    hipLaunchKernelGGL(k_near, dim3(G.light_blocks, Fs), dim3(256), 0, st, s.sorted, s.cmeta, s.nearb, s.counts, P);
    mark(c, s, st, ST_NEAR + 1);
    fid_launch_log("k_resolve", 1024, G.resolve_lds);
    hipLaunchKernelGGL(k_resolve, dim3(Fs), dim3(1024), G.resolve_lds, st, s.sorted, s.nearb, s.filtered, s.counts, s.worklist, s.nwork, P, G.near_words,
                       c->d_global, t.resolve_reg_max);
    mark(c, s, st, ST_RESOLVE + 1);
    chain_point(c, s, st, 5);
    // ---- K6
    fid_launch_log("k_identify", 64, G.ident_lds);
    hipLaunchKernelGGL(k_identify, dim3(G.ident_blocks), dim3(64), G.ident_lds, st, s.g, s.gfstride, s.filtered, s.worklist, s.nwork, c->d_dict, s.ident,
                       s.bits, P);
    mark(c, s, st, ST_IDENT + 1);
    // ---- K7
    fid_launch_log("k_filter_markers", 64, G.filter_lds);
    hipLaunchKernelGGL(k_filter_markers, dim3(Fs), dim3(64), G.filter_lds, st, s.filtered, s.ident, s.pre, s.counts, P, s.filter_scratch, t.filter_lds,
                       s.accsrc, s.mksrc);
    mark(c, s, st, ST_FILTER + 1);
    if (P.refine == 2)  // CORNER_REFINE_CONTOUR: a wave per marker fits the four sides of its contour (writes ids and corners)
        hipLaunchKernelGGL(k_refine_contour, dim3(P.maxMarkers < 64 ? P.maxMarkers : 64, Fs), dim3(64), 0, st, (const fid_marker *)s.pre, s.markers,
                           (const int *)s.mksrc, (const DevCand *)s.filtered, (const uint32_t *)s.dense, (const uint32_t *)s.tab, (const uint32_t *)s.pool,
                           s.counts, P);
    else {  // (the LDS and tap registers of k_subpix follow its window bound: an instantiation per bound, the smallest that holds the window)
#define SUBPIX_LAUNCH(BOUND)                                                                                                                        \
    {                                                                                                                                               \
        fid_launch_log("k_subpix<" #BOUND ">", 64, 0);                                                                                              \
        hipLaunchKernelGGL(k_subpix<BOUND>, dim3(G.subpix_blocks), dim3(64), 0, st, s.g, s.gfstride, s.pre, s.markers, s.counts, c->d_subpix_mask, P); \
    }
        if (P.subpixWin <= 5 && !t.subpix_win7) SUBPIX_LAUNCH(5)
        else if (P.subpixWin <= 7) SUBPIX_LAUNCH(7)
        else SUBPIX_LAUNCH(15)
#undef SUBPIX_LAUNCH
    }
    mark(c, s, st, ST_SUBPIX + 1);
    if (c->pose_req.ahead(c))  // (the remembered marker pose; where fid_pose_last_cov_cam was the last to ask, its covariance behind it)
        pose_launch(c, st, s.ev[EV_POSE0], s.ev[EV_POSE1], s.markers, &s.counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), nullptr, Fs, P.maxMarkers,
                    c->pose_req.ask, s.poses, s.pcov);
    chain_point(c, s, st, 99);
    return FID_OK;
}

fid_status enqueue_detect(fid_ctx *c, const uint8_t *d_src, int F, int W, int H, int stride, long long fstride, fid_encoding enc)
{
    {
        const fid_status rcv = check_call(c, F, W, H, stride, enc);
        if (rcv != FID_OK) return rcv;
    }
    const fid_ctx::Tuning &t = c->tune;
    const fid_ctx::Pending in = {d_src, F, W, H, stride, fstride, enc};
    hipStream_t st0 = c->stream;
    // ---- K0 geometry: mono8 device input is used in place (any stride); colour goes through k_to_gray
    const bool to_gray = enc != FID_ENC_MONO8;
    const int gstride = to_gray ? W : stride;
    const long long gfstride = to_gray ? (long long)W * H : fstride;
    const uint8_t *gray = to_gray ? c->d_gray : d_src;
    set_geometry(c, W, H, gstride, F);
    if (c->wait_ev) {
        HIPCHK(c, hipStreamWaitEvent(st0, c->wait_ev, 0));
        c->wait_ev = nullptr;
    }
    if (c->d_seedhash) {
        // a new generation makes every entry of the seed hash tables stale; clear them when the 10-bit number wraps
        if (++c->seed_gen > 1023) {
            HIPCHK(c, hipMemsetAsync(c->d_seedhash, 0, (size_t)c->lim.max_batch * c->seed_hash_cap * sizeof(unsigned long long), st0));
            c->seed_gen = 1;
        }
        c->P.seedGen = c->seed_gen;
    }
    // masks pad words must be zero; re-zero when the layout changes
    if (c->masks_W != W || c->masks_H != H || c->masks_S != c->P.nscales) {
        HIPCHK(c, hipMemsetAsync(c->d_masks, 0, c->masks_bytes, st0));
        c->masks_W = W;
        c->masks_H = H;
        c->masks_S = c->P.nscales;
    }
    layout_results(c, F);
    if (!c->res_precleared) HIPCHK(c, hipMemsetAsync(c->d_res, 0, c->res_clear_bytes, st0));  // global flags, work-list counters, per-frame counters
    c->res_precleared = false;
    // ---- the batch is cut into sub-batches that run the whole pipeline on their own streams: the latency-bound
    //      tail of one sub-batch's kernels (the longest border, the last candidates) overlaps the next one's bulk
    // (decided HERE and nowhere else: frames that come up from the host are cut by the copy's pieces whether or not the copy overlaps)
    c->piece_chain = t.pieces > 1 && !c->chained && !c->host_feed && !c->from_host_call && !c->whole_border_walk && t.sub_frames <= 0 &&
                     F >= 32 * t.pieces && t.stagger == 0;
    const SubPlan plan = plan_sub_batches(c, F);
    const int nsub = plan.nsub;
    const bool chainp = c->piece_chain, cycles = !c->whole_border_walk;
    c->last_nsub = nsub;
    c->tail_recorded = false;
    {
        const fid_status rcs = ensure_streams(c, nsub, F);
        if (rcs != FID_OK) return rcs;
    }
    SubBatch subs[fid_ctx::MAX_SUB];
    Grids grids[fid_ctx::MAX_SUB];
    for (int sb = 0; sb < nsub; sb++) {
        subs[sb] = sub_batch_view(c, plan, sb, d_src, fstride, gray, gfstride, W, H);
        grids[sb] = launch_grids(t, subs[sb].P, subs[sb].Fs);
    }
    if (nsub > 1) HIPCHK(c, hipEventRecord(c->fork_ev, st0));
    // a sub-batch's front, behind what it has to wait for
    auto front = [&](int sb) -> fid_status {
        hipStream_t st = subs[sb].st;
        if (nsub > 1) HIPCHK(c, hipStreamWaitEvent(st, c->fork_ev, 0));
        // (a chain of pieces: this one's threshold starts when the piece before it is through its find_starts)
        if (chainp && sb > 0) HIPCHK(c, hipStreamWaitEvent(st, c->fs_done[sb - 1], 0));
        if (c->host_feed) HIPCHK(c, hipStreamWaitEvent(st, c->in_ready[sb], 0));
        // staggered starts: the contour stage of a sub-batch (threshold ... approx) keeps the whole chip busy, what follows
        // (candidates, identification, corners) is a chain of short latency-bound kernels -- let the next sub-batch's contour
        // stage run under that tail instead of beside another contour stage
        if (nsub > 1 && t.stagger > 0 && sb >= t.stagger) HIPCHK(c, hipStreamWaitEvent(st, c->walk_done[sb - t.stagger], 0));
        return stage_front(c, subs[sb], grids[sb], in);
    };
    // its contour stage and candidate tail; the context's stream waits for its end
    auto rest = [&](int sb) -> fid_status {
        const SubBatch &s = subs[sb];
        if (cycles && nsub > 1 && t.fs_barrier && !chainp)
            for (int o = 0; o < nsub; o++)
                if (o != sb) HIPCHK(c, hipStreamWaitEvent(s.st, c->fs_done[o], 0));
        fid_status rc = cycles ? stage_cycle_tracing(c, s, grids[sb]) : stage_whole_border(c, s, grids[sb]);
        if (rc == FID_OK) rc = stage_tail(c, s, grids[sb]);
        if (rc != FID_OK) return rc;
        if (nsub > 1) {
            HIPCHK(c, hipEventRecord(c->sub_done[sb], s.tail));
            // (a chain of pieces: the context's stream carries the fronts of the even pieces -- it waits for the tails when all
            //  pieces are enqueued, below)
            if (!chainp) HIPCHK(c, hipStreamWaitEvent(st0, c->sub_done[sb], 0));
        }
        return FID_OK;
    };
    if (chainp) {
        // piece by piece: piece k + 2 goes behind piece k on the same two streams
        for (int sb = 0; sb < nsub; sb++) {
            fid_status rcs = front(sb);
            if (rcs == FID_OK) rcs = rest(sb);
            if (rcs != FID_OK) return rcs;
        }
        for (int sb = 0; sb < nsub; sb++) HIPCHK(c, hipStreamWaitEvent(st0, c->sub_done[sb], 0));
    } else {
        // The host enqueues in two rounds: first every sub-batch's front, then every sub-batch's rest.  (One round -- a whole
        // sub-batch, some thirty launches, before the next one's first kernel -- left the second sub-batch's stream empty for the
        // first 0.35 - 0.6 ms of every step.)
        for (int sb = 0; sb < nsub; sb++) {
            const fid_status rcs = front(sb);
            if (rcs != FID_OK) return rcs;
        }
        for (int sb = 0; sb < nsub; sb++) {
            const fid_status rcs = rest(sb);
            if (rcs != FID_OK) return rcs;
        }
    }
    const DevParams &P = c->P;
    HIPCHK(c, hipGetLastError());
    // ---- results
    c->pose_req.forget();
    c->map_req.forget();
    c->rob_req.forget();
    const bool map_ahead = c->map_req.ahead(c);
    const PoseAsk &ma = c->map_req.ask;
    if (map_ahead) {
        // the camera among the map's fiducials, a wave per frame, behind every sub-batch's k_pose
        map_pose_launch(c, st0, c->d_markers, &c->d_counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), P.maxMarkers, F, ma.cam, c->d_mposes, ma.cov,
                        ma.sigma, c->d_mcov);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(c->h_res, c->d_res, c->pose_req.ahead(c) ? c->res_poses_end : c->res_markers_end, hipMemcpyDeviceToHost, st0));  // one copy
    if (map_ahead) HIPCHK(c, hipMemcpyAsync(c->h_mposes, c->d_mposes, sizeof(fid_map_pose_out) * (size_t)F, hipMemcpyDeviceToHost, st0));
    if (map_ahead && ma.cov) HIPCHK(c, hipMemcpyAsync(c->h_mcov, c->d_mcov, sizeof(fid_map_pose_cov) * (size_t)F, hipMemcpyDeviceToHost, st0));
    if (c->rob_req.ahead(c)) {
        // fid_map_pose_robust_last_cam asked before: the consensus pose of these frames, for the same camera and options
        map_pose_robust_launch(c, st0, c->d_markers, &c->d_counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), P.maxMarkers, F, c->rob_req.ask.cam,
                               c->rob_req.ask.opts, c->d_rposes, c->d_mrob);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_rposes, c->d_rposes, sizeof(fid_map_pose_out) * (size_t)F, hipMemcpyDeviceToHost, st0));
        HIPCHK(c, hipMemcpyAsync(c->h_mrob, c->d_mrob, sizeof(fid_map_robust_out) * (size_t)F, hipMemcpyDeviceToHost, st0));
    }
    c->last_frames = F;
    c->last_W = W;
    c->last_H = H;
    c->last_gray = gray;
    c->last_gfstride = gfstride;
    c->pend = in;
    c->in_flight = true;
    c->chained = false;
    c->wait_ev = nullptr;       // fid_order_after holds for ONE submit: the other context's events are not kept beyond it (it may
    c->wait_copy_ev = nullptr;  // be destroyed before this context's next call)
    c->fed_from_host = false;  // (feed_and_enqueue sets it after this call)
    return FID_OK;
}

// k_pose for F frames of per_frame markers on a stream, for a.cov with k_pose_cov behind it; under FID_PROFILE between two events
void pose_launch(fid_ctx *c, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, const fid_marker *d_markers, const int *d_n, int n_stride_ints,
                 const double *d_lens, int F, int per_frame, const PoseAsk &a, fid_pose_out *d_out, fid_pose_cov *d_cov)
{
    const PoseCam cam = pose_cam_from(a.cam, a.len);
    int blocks = (F * per_frame + 7) / 8;  // eight lanes per marker, eight markers per wave
    blocks = blocks < 1 ? 1 : (blocks > 256 * 16 ? 256 * 16 : blocks);
    if (c->profile) (void)hipEventRecord(ev0, st);
    POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_pose<CAM_MODEL>, dim3(blocks), dim3(64), 0, st, d_markers, d_n, n_stride_ints, d_lens, F,
                                                    per_frame, cam, d_out));
    if (a.cov)
        POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_pose_cov<CAM_MODEL>, dim3(blocks), dim3(64), 0, st, d_markers, d_n, n_stride_ints, d_lens, F,
                                                        per_frame, cam, (const fid_pose_out *)d_out, a.sigma, d_cov));
    if (c->profile) (void)hipEventRecord(ev1, st);
}

fid_status run_detect(fid_ctx *c, const uint8_t *d_src, int F, int W, int H, int stride, long long fstride, fid_encoding enc,
                      fid_marker *out, int cap_per_frame, int *n_per_frame);

fid_status finish_detect(fid_ctx *c, fid_marker *out, int cap_per_frame, int *n_per_frame)
{
    const DevParams &P = c->P;
    const int F = c->pend.F;
    c->in_flight = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pose_req.finished(c);
    c->map_req.finished(c);
    c->rob_req.finished(c);
    if (c->profile) {
        // a stage's time = its event-bracketed time on its own stream, summed over the sub-batches (with more than
        // one sub-batch the brackets of different streams overlap in wall time)
        for (int i = 0; i < ST_COUNT; i++) c->stage_ms[i] = 0.f;
        for (int sb = 0; sb < c->last_nsub; sb++)
            for (int i = 0; i <= ST_SUBPIX; i++) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, c->sub_ev[sb][i], c->sub_ev[sb][i + 1]) == hipSuccess) c->stage_ms[i] += ms;
            }
        if (!c->whole_border_walk)  // the seed walk, and the seedless chain beside it on the auxiliary streams
            for (int sb = 0; sb < c->last_nsub; sb++) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, c->sub_ev[sb][EV_SEEDWALK0], c->sub_ev[sb][EV_SEEDWALK1]) == hipSuccess) c->stage_ms[ST_SEEDWALK] += ms;
                if (hipEventElapsedTime(&ms, c->sub_ev[sb][EV_SEEDLESS0], c->sub_ev[sb][EV_SEEDLESS1]) == hipSuccess) c->stage_ms[ST_SEEDLESS] += ms;
                if (c->pose_req.at_hand && hipEventElapsedTime(&ms, c->sub_ev[sb][EV_POSE0], c->sub_ev[sb][EV_POSE1]) == hipSuccess) c->stage_ms[ST_POSE] += ms;
            }
    }
#ifdef FID_DEBUG_STATS
    {
        const unsigned long long *d = c->h_global->dbg;
        fprintf(stderr, "walk stats: ranges %llu iters %llu ckpts %llu (forced %llu) active-lanes/iter %.1f cyc/range %.0f ckpt-cyc/range %.0f wait-cyc/range %.0f\n",
                d[7], d[0], d[1], d[5], d[0] ? (double)d[2] / d[0] : 0., d[7] ? (double)d[6] / d[7] : 0., d[7] ? (double)d[3] / d[7] : 0.,
                d[7] ? (double)d[4] / d[7] : 0.);
        fprintf(stderr, "walk waves %llu: total cyc avg %.0f max %llu; own queue dry at avg %.0f max %llu\n", d[12],
                d[12] ? (double)d[8] / d[12] : 0., d[9], d[12] ? (double)d[10] / d[12] : 0., d[11]);
        fprintf(stderr, "walk longest %llu steps, total steps %llu\n", d[13], d[14]);
        fprintf(stderr, "resolve (frame 0, n %llu, %llu label rounds) cycles: load %llu label %llu count %llu components %llu places %llu move %llu\n", d[31] >> 32,
                d[31] & 0xffffffffull, d[25], d[26], d[27], d[28], d[29], d[30]);
        if (d[1])
            fprintf(stderr, "checkpoint cycles: wait %.0f activate %.0f retire %.0f hand-out %.0f chunks %.0f refill %.0f; lanes at a checkpoint: need %.1f loading %.1f final %.1f idle %.1f\n",
                    (double)d[4] / d[1], (double)d[16] / d[1], (double)d[17] / d[1], (double)d[18] / d[1], (double)d[19] / d[1], (double)d[20] / d[1],
                    (double)d[21] / d[1], (double)d[22] / d[1], (double)d[23] / d[1], (double)d[24] / d[1]);
    }
#endif
    if (!c->whole_border_walk && (c->h_global->overflow & (2u | 8u))) {
        // the tracing seeds and their points scale with the total border length of the frame, texture included: when they
        // do not fit max_contours_per_frame / max_points_per_frame, trace this call with the whole-border walk, which only
        // needs room for the probe survivors
        if (getenv("FID_VERBOSE"))
            fprintf(stderr, "fid: seed tracing overflow flags 0x%x (frame 0: seeds %d starts %d surv %d chunks %d; maxContours %d maxChunks %d shift %d): whole-border walk\n",
                    c->h_global->overflow, c->h_counts[0].nseeds, c->h_counts[0].nstarts, c->h_counts[0].nsurv, c->h_counts[0].npool, c->P.maxContours,
                    c->P.maxChunks, c->P.seedShift);
        c->whole_border_walk = true;
        c->fallbacks++;
        const fid_ctx::Pending pd = c->pend;
        const fid_status rc2 = run_detect(c, pd.d_src, pd.F, pd.W, pd.H, pd.stride, pd.fstride, pd.enc, out, cap_per_frame, n_per_frame);
        c->whole_border_walk = false;
        return rc2;
    }
    fid_status rc = FID_OK;
    if (c->h_global->overflow) {
        const unsigned ov = c->h_global->overflow;
        // which table: so that the caller knows which limit to raise
        c->last_error = "internal capacity exceeded:";
        if (ov & 1u) c->last_error += " max_starts_per_frame";
        if (ov & 2u) c->last_error += " max_contours_per_frame";
        if (ov & 8u) c->last_error += " max_points_per_frame";
        c->last_error += " (raise fid_limits)";
        rc = FID_E_CAPACITY;
    }
    for (int f = 0; f < F; f++) {
        int n = c->h_counts[f].nmark;
        if (c->h_counts[f].overflow & 3) {
            c->last_error = "per-frame candidate/marker capacity exceeded: raise fid_limits";
            rc = FID_E_CAPACITY;
        }
        if (c->h_counts[f].overflow & 4) {
            // CORNER_REFINE_CONTOUR on a marker with a side of fewer than two contour points: cv::solve throws inside
            // aruco::detectMarkers, imageCallback's catch(cv::Exception&) logs it and publishes nothing for the frame
            if (rc == FID_OK) {
                rc = FID_E_CV_EXCEPTION;
                c->last_error = "cv exception: the reference's detectMarkers throws on frame " + std::to_string(f) +
                                " (CORNER_REFINE_CONTOUR: a marker side of fewer than two contour points)";
            }
            n_per_frame[f] = -1;
            continue;
        }
        if (n > cap_per_frame) {
            n = cap_per_frame;
            c->last_error = "caller marker capacity too small";
            rc = FID_E_CAPACITY;
        }
        n_per_frame[f] = n;
        memcpy(out + (size_t)f * cap_per_frame, c->h_markers + (size_t)f * P.maxMarkers, sizeof(fid_marker) * n);
    }
    return rc;
}

fid_status run_detect(fid_ctx *c, const uint8_t *d_src, int F, int W, int H, int stride, long long fstride, fid_encoding enc,
                      fid_marker *out, int cap_per_frame, int *n_per_frame)
{
    if (refuse_in_flight(c) || !out || !n_per_frame || cap_per_frame < 0) {
        c->wait_ev = c->wait_copy_ev = nullptr;  // (fid_order_after holds for one call, refused or not)
        c->chained = false;
        return FID_E_INVALID_ARG;
    }
    c->blocking = true;
    const fid_status rc = enqueue_detect(c, d_src, F, W, H, stride, fstride, enc);
    c->blocking = false;
    if (rc != FID_OK) {
        c->wait_ev = c->wait_copy_ev = nullptr;
        c->chained = false;
        if (c->last_frames > 0 && !c->in_flight) layout_results(c, c->last_frames);  // (the layout of the last call that ran)
        return rc;
    }
    return finish_detect(c, out, cap_per_frame, n_per_frame);
}

// The launch tunables of a context, from the environment: read once, here, when the context is created
fid_ctx::Tuning read_tuning()
{
    fid_ctx::Tuning t;
    auto num = [](const char *name, int *v) {  // (a variable that is not set leaves the default)
        const char *e = getenv(name);
        if (e) *v = atoi(e);
        return e != nullptr;
    };
    int v = 0;
    num("FID_SUB_FRAMES", &t.sub_frames);
    if (const char *e = getenv("FID_SUB_SHARES")) {
        t.sub_shares_set = true;
        t.n_sub_share = 0;
        for (const char *q = e; *q && t.n_sub_share < fid_ctx::MAX_SUB;) {
            if (atoi(q) > 0) t.sub_share[t.n_sub_share++] = atoi(q);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
    }
    if (const char *e = getenv("FID_FEED_SHARES")) (void)sscanf(e, "%d,%d,%d,%d", &t.feed_share[0], &t.feed_share[1], &t.feed_share[2], &t.feed_share[3]);
    num("FID_PIECES", &t.pieces);
    num("FID_STAGGER", &t.stagger);
    num("FID_FS_BARRIER", &t.fs_barrier);
    num("FID_CHAIN_AT", &t.chain_at);
    t.idx_stream = getenv("FID_NO_IDX_STREAM") == nullptr;
    if (num("FID_PRIO", &v)) t.prio = v != 0;
    if (num("FID_THR_NW", &v)) t.thr_nw = v == 3 ? 3 : 5;
    if (num("FID_THR_SPLIT", &v)) t.thr_split = v != 0;
    num("FID_THR_ROWS", &t.thr_rows);
    if (num("FID_THR_XCD", &v)) t.thr_xcd = v != 0;
    num("FID_SEED_SHIFT", &t.seed_shift);
    if (const char *e = getenv("FID_SEED_KERNEL")) t.seed_kernel = !strcmp(e, "split") ? 1 : (!strcmp(e, "fused") ? 2 : 0);
    t.trace_legacy = getenv("FID_TRACE") && !strcmp(getenv("FID_TRACE"), "legacy");
    if (num("FID_WALK_BLOCKS", &v) && v > 0) t.walk_blocks = v;
    num("FID_WALK_CAP", &t.walk_blocks_cap);
    num("FID_WALK2_DIV", &t.walk2_div);
    num("FID_SW_BLOCKS", &t.sw_blocks);
    num("FID_COPY_BLOCKS", &t.copy_blocks);
    num("FID_PROBE_REFILL", &t.probe_refill);
    num("FID_PROBE_REFILL0", &t.probe_refill0);
    if (num("FID_PROBE_PASSES", &v) && (v == 1 || v == 2)) t.probe_passes = v;  // (1 or 2; anything else leaves the default)
    if (num("FID_PROBE_SINGLE", &v)) t.probe_single = v < 1 ? 1 : (v > 64 ? 64 : v);  // (1 ... 64 workgroups a frame, the range of the sweep; clamped)
    t.segc_warm = getenv("FID_NO_SEGC_WARM") ? 0 : 1;
    if (num("FID_LIGHT_X", &v)) t.light_x = v > 0 ? v : 1;
    num("FID_RESOLVE_LDS", &t.resolve_lds_kb);
    num("FID_RESOLVE_SERIAL", &t.resolve_serial);
    if (num("FID_RESOLVE_REG_MAX", &v)) t.resolve_reg_max = v < 0 ? 0 : (v > 64 ? 64 : v);
    num("FID_TAIL_GRID", &t.tail_grid);
    if (num("FID_SUBPIX_WIN7", &v)) t.subpix_win7 = v != 0;
    if (num("FID_FILTER_LDS", &v)) t.filter_lds = v > 0 ? v : 1;
    return t;
}

}  // namespace

extern "C" {

void fid_default_params(fid_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    // node defaults: aruco_detect.cpp:690-727
    p->adaptiveThreshConstant = 7;
    p->adaptiveThreshWinSizeMin = 3;
    p->adaptiveThreshWinSizeMax = 53;
    p->adaptiveThreshWinSizeStep = 4;
    p->cornerRefinementMethod = 1;
    p->cornerRefinementWinSize = 5;
    p->cornerRefinementMaxIterations = 30;
    p->cornerRefinementMinAccuracy = 0.01;
    p->errorCorrectionRate = 0.6;
    p->minCornerDistanceRate = 0.05;
    p->markerBorderBits = 1;
    p->minDistanceToBorder = 3;
    p->maxErroneousBitsInBorderRate = 0.04;
    p->minMarkerDistanceRate = 0.05;
    p->minMarkerPerimeterRate = 0.1;
    p->maxMarkerPerimeterRate = 4.0;
    p->minOtsuStdDev = 5.0;
    p->perspectiveRemoveIgnoredMarginPerCell = 0.13;
    p->perspectiveRemovePixelPerCell = 8;
    p->polygonalApproxAccuracyRate = 0.01;
}

void fid_default_limits(fid_limits *l)
{
    if (!l) return;
    memset(l, 0, sizeof(*l));
    l->max_width = 1920;
    l->max_height = 1080;
    l->max_batch = 1;
    l->max_starts_per_frame = 262144;
    l->max_contours_per_frame = 16384;
    l->max_candidates_per_frame = 2048;
    l->max_markers_per_frame = 256;
    l->max_points_per_frame = 4 * 1024 * 1024;
}

fid_status fid_create(const fid_params *params, const fid_dict *dict, const fid_limits *limits, int device, fid_ctx **out)
{
    if (!params || !dict || !out || !dict->bytes || dict->n_markers <= 0 || dict->marker_size < 3 || dict->marker_size > 7)
        return FID_E_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FID_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return FID_E_INVALID_ARG;
    fid_ctx *c = new (std::nothrow) fid_ctx();
    if (!c) return FID_E_OUT_OF_MEMORY;
    c->device = device;
    fid_limits L;
    fid_default_limits(&L);
    if (limits) {
        if (limits->max_width > 0) L.max_width = limits->max_width;
        if (limits->max_height > 0) L.max_height = limits->max_height;
        if (limits->max_batch > 0) L.max_batch = limits->max_batch;
        if (limits->max_starts_per_frame > 0) L.max_starts_per_frame = limits->max_starts_per_frame;
        if (limits->max_contours_per_frame > 0) L.max_contours_per_frame = limits->max_contours_per_frame;
        if (limits->max_candidates_per_frame > 0) L.max_candidates_per_frame = limits->max_candidates_per_frame;
        if (limits->max_markers_per_frame > 0) L.max_markers_per_frame = limits->max_markers_per_frame;
        if (limits->max_points_per_frame > 0) L.max_points_per_frame = limits->max_points_per_frame;
    }
    // contexts for a few frames at a time (the node's shape, max_batch 1) get room for the denser seed grid by default
    if (L.max_batch <= 4) {
        if (!limits || limits->max_contours_per_frame <= 0) L.max_contours_per_frame = 65536;
        if (!limits || limits->max_points_per_frame <= 0) L.max_points_per_frame = 16 * 1024 * 1024;
    } else if (L.max_batch <= 16) {
        if (!limits || limits->max_contours_per_frame <= 0) L.max_contours_per_frame = 32768;
        if (!limits || limits->max_points_per_frame <= 0) L.max_points_per_frame = 8 * 1024 * 1024;
    }
    L.max_candidates_per_frame = roundup(L.max_candidates_per_frame, 32);
    if (L.max_candidates_per_frame > 4096 || L.max_batch > 65535 || L.max_markers_per_frame > L.max_candidates_per_frame ||
        L.max_contours_per_frame > (1 << 20)) {  // (seed indices are 20-bit fields of the SeedHash entries)
        delete c;
        return FID_E_INVALID_ARG;
    }
    c->lim = L;
    c->dict_ms = dict->marker_size;
    c->dict_maxc = dict->max_correction_bits;
    c->dict_n = dict->n_markers;
    size_t dbytes = (size_t)dict->n_markers * 4 * ((dict->marker_size * dict->marker_size + 7) / 8);
    c->dict_host.assign(dict->bytes, dict->bytes + dbytes);
    c->profile = getenv("FID_PROFILE") && atoi(getenv("FID_PROFILE")) != 0;
    c->tune = read_tuning();
    c->whole_border_walk = c->tune.trace_legacy;
    memset(&c->P, 0, sizeof(c->P));

    fid_status rc = FID_OK;
    auto fail = [&](fid_status s) {
        fid_destroy(c);
        return s;
    };
#define TRY(expr)                         \
    do {                                  \
        rc = (expr);                      \
        if (rc != FID_OK) return fail(rc); \
    } while (0)
#define TRYHIP(expr)                                   \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) {                        \
            fprintf(stderr, "fid_create: %s: %s\n", #expr, hipGetErrorString(e_)); \
            return fail(e_ == hipErrorOutOfMemory ? FID_E_OUT_OF_MEMORY : FID_E_HIP); \
        }                                              \
    } while (0)
    TRYHIP(hipSetDevice(device));
    TRYHIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : c->pose_ev) TRYHIP(hipEventCreate(&e));
    TRYHIP(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
    TRYHIP(hipEventCreateWithFlags(&c->tail_ev, hipEventDisableTiming));
    int prio_lo = 0, prio_hi = 0;  // (numerically lower = more urgent)
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    for (int sb = 0; sb < fid_ctx::MAX_SUB; sb++) {
        int prio = c->tune.prio ? prio_hi + sb : prio_lo;
        if (prio > prio_lo) prio = prio_lo;
        // (the sub-batch and auxiliary streams themselves are made when a call first needs them -- ensure_streams(): every live
        //  stream is a claim on the hardware queues; eighteen idle ones per context cost the STag path its rate in round 2, and
        //  creating eight more for an experiment cost this path a quarter of its own)
        c->sub_prio[sb] = prio;
        TRYHIP(hipEventCreateWithFlags(&c->aux_fork[sb], hipEventDisableTiming));
        TRYHIP(hipEventCreateWithFlags(&c->aux_join[sb], hipEventDisableTiming));
        TRYHIP(hipEventCreateWithFlags(&c->sub_done[sb], hipEventDisableTiming));
        TRYHIP(hipEventCreateWithFlags(&c->walk_done[sb], hipEventDisableTiming));
        TRYHIP(hipEventCreateWithFlags(&c->in_ready[sb], hipEventDisableTiming));
        TRYHIP(hipEventCreateWithFlags(&c->fs_done[sb], hipEventDisableTiming));
        TRYHIP(hipEventCreateWithFlags(&c->front_done[sb], hipEventDisableTiming));
        TRYHIP(hipEventCreateWithFlags(&c->aux_idx[sb], hipEventDisableTiming));
        for (hipEvent_t &e : c->sub_ev[sb]) TRYHIP(hipEventCreate(&e));
    }
    const size_t F = L.max_batch, MC = L.max_candidates_per_frame, MM = L.max_markers_per_frame;
    TRY(dalloc(c, &c->d_subpix_mask, (size_t)(2 * SP_MAXWIN_MAX + 1) * (2 * SP_MAXWIN_MAX + 1)));
    TRY(dalloc(c, &c->d_probe_tables, (size_t)4096));
    hipLaunchKernelGGL(k_probe_tables, dim3(1), dim3(256), 0, nullptr, c->d_probe_tables);
    TRYHIP(hipGetLastError());
    TRYHIP(hipDeviceSynchronize());
    TRY(dalloc(c, &c->d_dict, dbytes));
    TRYHIP(hipMemcpy(c->d_dict, c->dict_host.data(), dbytes, hipMemcpyHostToDevice));
    rc = apply_params(c, params);
    if (rc != FID_OK) return fail(rc);
    TRY(dalloc(c, &c->d_gray, F * L.max_width * L.max_height));
    c->masks_bytes = masks_elems(c, L.max_width, L.max_height, (int)F) * sizeof(uint32_t);
    // a narrower image can need a larger padded pitch only through rounding; keep a margin
    c->masks_bytes += (size_t)F * c->P.nscales * (L.max_height + 2) * 16 * sizeof(uint32_t);
    TRYHIP(hipMalloc((void **)&c->d_masks, c->masks_bytes));
    TRY(dalloc(c, &c->d_starts, F * L.max_starts_per_frame));
    TRY(dalloc(c, &c->d_surv1, F * L.max_starts_per_frame));
    TRY(dalloc(c, &c->d_surv, F * L.max_starts_per_frame));
    c->max_chunks = (L.max_points_per_frame + CK - 1) / CK;
    TRY(dalloc(c, &c->d_pool, F * (size_t)c->max_chunks * CKW));
    if (!c->whole_border_walk) {
        TRY(dalloc(c, &c->d_segs, F * L.max_contours_per_frame));
        TRY(dalloc(c, &c->d_pend, F * L.max_contours_per_frame));
        TRY(dalloc(c, &c->d_seedq, F * L.max_contours_per_frame));
        c->seed_hash_cap = 1;
        while (c->seed_hash_cap < 2 * L.max_contours_per_frame) c->seed_hash_cap *= 2;
        TRY(dalloc(c, &c->d_seedhash, F * (size_t)c->seed_hash_cap));
        TRYHIP(hipMemset(c->d_seedhash, 0, F * (size_t)c->seed_hash_cap * sizeof(unsigned long long)));
        TRY(dalloc(c, &c->d_wres, F * L.max_contours_per_frame));
        TRY(dalloc(c, &c->d_cinfo, F * L.max_contours_per_frame));
        TRY(dalloc(c, &c->d_cbase, F * L.max_contours_per_frame));
        TRY(dalloc(c, &c->d_recs, 2 * F * L.max_contours_per_frame));
        TRY(dalloc(c, &c->d_dense, F * (size_t)c->max_chunks * (CK / 4) + 2));  // (+ 8 bytes: k_approx reads a contour's last codes eight at a time)
    }
    TRY(dalloc(c, &c->d_contours, F * L.max_contours_per_frame));
    {
        int maxdim = L.max_width > L.max_height ? L.max_width : L.max_height;
        size_t nck = (size_t)(params->maxMarkerPerimeterRate * maxdim) / 64 + 4;
        c->ckpts_elems = F * 2 * L.max_contours_per_frame * nck;  // rows: seeds, then survivors
        TRY(dalloc(c, &c->d_ckpts, c->ckpts_elems));
    }
    TRY(dalloc(c, &c->d_cands, F * MC));
    TRY(dalloc(c, &c->d_sorted, F * MC));
    TRY(dalloc(c, &c->d_cmeta, F * MC));
    TRY(dalloc(c, &c->d_filtered, F * MC));
    TRY(dalloc(c, &c->d_near, F * MC * (MC / 32)));
    TRY(dalloc(c, &c->d_ident, F * MC));
    // (the cell bits: room for any grid of up to 9 cells -- every 7x7 or smaller dictionary with a 1-cell border -- or the one the
    //  parameters ask for; fid_set_params grows it)
    {
        const int msb = c->P.markerSize + 2 * c->P.borderBits;
        c->bits_cap = msb * msb > 81 ? msb * msb : 81;
        TRY(dalloc(c, &c->d_bits, F * MC * c->bits_cap));
    }
    TRY(dalloc(c, &c->d_pre, F * MM));
    TRY(dalloc(c, &c->d_filter_scratch, F * MC));
    TRY(dalloc(c, &c->d_accsrc, F * MC));
    TRY(dalloc(c, &c->d_mksrc, F * MM));
    TRY(dalloc(c, &c->d_res, results_bytes((int)F, (int)MM)));
    TRY(dalloc(c, &c->d_worklist, F * MC));
    TRY(dalloc(c, &c->d_pose_n, 1));
    TRYHIP(hipHostMalloc((void **)&c->h_res, results_bytes((int)F, (int)MM), hipHostMallocDefault));
    memset(c->h_res, 0, results_bytes((int)F, (int)MM));
    layout_results(c, (int)F);
    TRYHIP(hipMemset(c->d_masks, 0, c->masks_bytes));
    // opt in to large dynamic LDS where needed
    TRYHIP(hipFuncSetAttribute((const void *)k_threshold<TX, TY, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));
    TRYHIP(hipFuncSetAttribute((const void *)k_approx, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
    TRYHIP(hipFuncSetAttribute((const void *)k_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    TRYHIP(hipFuncSetAttribute((const void *)k_threshold_wide<THRW_NT, THRW_WT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)((8191 + 1 + THRW_NT / 64) * sizeof(unsigned long long))));
    TRYHIP(hipFuncSetAttribute((const void *)k_identify, hipFuncAttributeMaxDynamicSharedMemorySize, FID_MAX_PATCH * FID_MAX_PATCH));
    TRYHIP(hipFuncSetAttribute((const void *)k_filter_markers, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
#undef TRY
#undef TRYHIP
    *out = c;
    return FID_OK;
}

void fid_destroy(fid_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void *dev[] = {c->d_gray, c->d_masks, c->d_starts, c->d_surv1, c->d_surv, c->d_pool, c->d_segs, c->d_pend, c->d_seedq, c->d_seedhash, c->d_wres, c->d_cinfo, c->d_cbase, c->d_filter_scratch, c->d_accsrc, c->d_mksrc, c->d_dense, c->d_recs, c->d_contours, c->d_ckpts, c->d_cands, c->d_sorted, c->d_cmeta, c->d_filtered, c->d_near,
                   c->d_ident, c->d_bits, c->d_pre, c->d_res, c->d_worklist, c->d_dict,
                   c->d_subpix_mask, c->d_probe_tables, c->d_pose_n};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    calib_free(c);
    build_free(c);
    charuco_free(c);
    calib_pts_free(c);
    diamond_free(c);
    rig_free(c);
    if (c->h_res) (void)hipHostFree(c->h_res);
    for (hipEvent_t e : c->pose_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->tail_ev) (void)hipEventDestroy(c->tail_ev);
    for (int sb = 0; sb < fid_ctx::MAX_SUB; sb++) {
        if (c->sub_stream[sb]) (void)hipStreamSynchronize(c->sub_stream[sb]);
        if (sb == 0 && c->idx_stream) {
            (void)hipStreamSynchronize(c->idx_stream);
            (void)hipStreamDestroy(c->idx_stream);
            c->idx_stream = nullptr;
        }
        if (c->aux_stream[sb]) {
            (void)hipStreamSynchronize(c->aux_stream[sb]);
            (void)hipStreamDestroy(c->aux_stream[sb]);
        }
        if (c->aux_fork[sb]) (void)hipEventDestroy(c->aux_fork[sb]);
        if (c->aux_join[sb]) (void)hipEventDestroy(c->aux_join[sb]);
        if (c->aux_idx[sb]) (void)hipEventDestroy(c->aux_idx[sb]);
        if (c->sub_done[sb]) (void)hipEventDestroy(c->sub_done[sb]);
        if (c->walk_done[sb]) (void)hipEventDestroy(c->walk_done[sb]);
        if (c->in_ready[sb]) (void)hipEventDestroy(c->in_ready[sb]);
        if (c->fs_done[sb]) (void)hipEventDestroy(c->fs_done[sb]);
        if (c->front_done[sb]) (void)hipEventDestroy(c->front_done[sb]);
        for (hipEvent_t e : c->sub_ev[sb])
            if (e) (void)hipEventDestroy(e);
        if (c->sub_stream[sb] && c->sub_stream[sb] != c->stream) (void)hipStreamDestroy(c->sub_stream[sb]);
    }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

fid_status fid_set_params(fid_ctx *c, const fid_params *p)
{
    if (!c || !p || c->in_flight) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int old_scales = c->P.nscales;
    fid_params keep = c->params;
    fid_status rc = apply_params(c, p);
    if (rc == FID_OK && c->P.nscales > old_scales) {
        // the masks buffer was sized for the scale count at creation (plus a margin): a larger scale count must fit
        size_t need = masks_elems(c, c->lim.max_width, c->lim.max_height, c->lim.max_batch) * sizeof(uint32_t);
        if (need > c->masks_bytes) {
            (void)apply_params(c, &keep);
            c->last_error = "more threshold scales than the context was created for";
            return FID_E_UNSUPPORTED;
        }
    }
    if (rc == FID_OK) {
        // what run_detect would refuse on every later frame is refused here, at reconfigure time: the chunk table was sized
        // for the creation-time maxMarkerPerimeterRate, and contour points live in LDS
        const int maxdim = c->lim.max_width > c->lim.max_height ? c->lim.max_width : c->lim.max_height;
        const unsigned maxPerim = (unsigned)(p->maxMarkerPerimeterRate * maxdim);
        DevParams Q = c->P;
        Q.maxPerim = (int)maxPerim;
        if (maxPerim > 36000u ||
            (size_t)c->lim.max_batch * 2 * c->lim.max_contours_per_frame * chunk_tab_pitch(Q) > c->ckpts_elems) {
            (void)apply_params(c, &keep);
            c->last_error = "maxMarkerPerimeterRate larger than the context was created for";
            return FID_E_UNSUPPORTED;
        }
    }
    if (rc == FID_OK) {
        // a wider grid than the cell-bits array has room for: grow it (nothing is in flight here)
        const int msb = c->P.markerSize + 2 * c->P.borderBits;
        if (msb * msb > c->bits_cap) {
            uint8_t *nb = nullptr;
            const hipError_t e = hipMalloc((void **)&nb, (size_t)c->lim.max_batch * c->lim.max_candidates_per_frame * msb * msb);
            if (e != hipSuccess) {
                (void)apply_params(c, &keep);
                c->last_error = std::string("hipMalloc (cell bits): ") + hipGetErrorString(e);
                return e == hipErrorOutOfMemory ? FID_E_OUT_OF_MEMORY : FID_E_HIP;
            }
            HIPCHK(c, hipFree(c->d_bits));
            c->d_bits = nb;
            c->bits_cap = msb * msb;
        }
    }
    if (rc != FID_OK) (void)apply_params(c, &keep);
    c->masks_W = 0;  // force re-zero
    return rc;
}

fid_status fid_detect_device(fid_ctx *c, const void *d_imgs, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                             int64_t frame_stride, fid_encoding enc, fid_marker *out, int32_t cap_per_frame, int32_t *n_per_frame)
{
    if (!c) return FID_E_INVALID_ARG;
    const hipError_t dev_rc = d_imgs ? hipSetDevice(c->device) : hipSuccess;
    if (!d_imgs || dev_rc != hipSuccess) {
        c->wait_ev = c->wait_copy_ev = nullptr;  // (fid_order_after holds for one call, refused or not)
        c->chained = false;
        if (!d_imgs) return FID_E_INVALID_ARG;
        c->last_error = std::string("hipSetDevice: ") + hipGetErrorString(dev_rc);  // a runtime failure is not an argument error
        return FID_E_HIP;
    }
    return run_detect(c, (const uint8_t *)d_imgs, nframes, width, height, stride, frame_stride, enc, out, cap_per_frame, n_per_frame);
}

fid_status fid_submit_device(fid_ctx *c, const void *d_imgs, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                             int64_t frame_stride, fid_encoding enc)
{
    if (!c) return FID_E_INVALID_ARG;
    fid_status rc = FID_E_INVALID_ARG;
    const bool was_in_flight = refuse_in_flight(c);
    if (!was_in_flight && d_imgs) {
        const hipError_t dev_rc = hipSetDevice(c->device);
        if (dev_rc == hipSuccess) rc = enqueue_detect(c, (const uint8_t *)d_imgs, nframes, width, height, stride, frame_stride, enc);
        else {
            c->last_error = std::string("hipSetDevice: ") + hipGetErrorString(dev_rc);
            rc = FID_E_HIP;
        }
    }
    c->wait_ev = nullptr;  // (fid_order_after holds for one submit, refused or not)
    c->wait_copy_ev = nullptr;
    c->chained = false;
    if (rc != FID_OK && !was_in_flight && c->last_frames > 0) layout_results(c, c->last_frames);
    return rc;
}

fid_status fid_order_after(fid_ctx *c, fid_ctx *prev)
{
    if (!c || c == prev || c->in_flight || (prev && prev->device != c->device)) return FID_E_INVALID_ARG;
    c->wait_ev = prev && prev->in_flight ? prev->tail_ev : nullptr;
    c->wait_copy_ev = prev && prev->in_flight && prev->fed_from_host && prev->last_nsub >= 1 ? prev->in_ready[prev->last_nsub - 1] : nullptr;
    c->chained = prev != nullptr;
    return FID_OK;
}

fid_status fid_collect(fid_ctx *c, fid_marker *out, int32_t cap_per_frame, int32_t *n_per_frame)
{
    if (!c || !out || !n_per_frame || cap_per_frame < 0) return FID_E_INVALID_ARG;
    if (!c->in_flight) {
        c->last_error = "nothing was submitted";
        return FID_E_INVALID_ARG;
    }
    HIPCHK(c, hipSetDevice(c->device));
    return finish_detect(c, out, cap_per_frame, n_per_frame);
}

// frames in host memory: the copies go on the copy stream, the pipeline is enqueued behind them (fid_detect_batch, fid_submit_batch)
// fid_order_after holds for ONE submit, refused or not: the other context's events are not kept beyond it (that context may be
// destroyed before this one's next call), and a refused call leaves no result layout of its own behind (fid_pose_last /
// fid_tap_read address the result block through last_frames).
static void drop_order_and_layout(fid_ctx *c, bool layout_touched)
{
    c->wait_ev = c->wait_copy_ev = nullptr;
    c->chained = false;
    if (layout_touched) {
        if (c->last_frames > 0) layout_results(c, c->last_frames);
        c->res_precleared = false;
    }
}

static fid_status feed_and_enqueue_impl(fid_ctx *c, const uint8_t *imgs, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                                        int64_t frame_stride, fid_encoding enc);

static fid_status feed_and_enqueue(fid_ctx *c, const uint8_t *imgs, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                                   int64_t frame_stride, fid_encoding enc)
{
    if (!c) return FID_E_INVALID_ARG;
    const fid_status rc = feed_and_enqueue_impl(c, imgs, nframes, width, height, stride, frame_stride, enc);
    if (rc != FID_OK) drop_order_and_layout(c, true);
    return rc;
}

static fid_status feed_and_enqueue_impl(fid_ctx *c, const uint8_t *imgs, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                                        int64_t frame_stride, fid_encoding enc)
{
    if (!c || !imgs || nframes < 1 || height < 1 || stride < 1) return FID_E_INVALID_ARG;
    if (nframes > c->lim.max_batch || refuse_in_flight(c)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (frame_stride < (int64_t)stride * height) return FID_E_INVALID_ARG;
    {
        // geometry, encoding and limits BEFORE any copy is queued: a refused call leaves no DMA from the caller's buffer behind
        const fid_status rcv = check_call(c, nframes, width, height, stride, enc);
        if (rcv != FID_OK) {
            c->wait_ev = c->wait_copy_ev = nullptr;
            c->chained = false;
            return rcv;
        }
    }
    size_t need = (size_t)frame_stride * (nframes - 1) + (size_t)stride * height;
    HIPCHK(c, c->in.reserve(need));
    // The frames go up in the pieces run_detect works in, one asynchronous copy per sub-batch on the copy stream with an event
    // behind it; a sub-batch's stream waits for its own event only, so the copy of sub-batch k + 1 runs under the kernels of
    // sub-batch k (pinned host memory -- a capture ring buffer -- copies at link speed; pageable memory is staged by the runtime
    // and copies more slowly, the overlap is the same).  A batch of a chain (fid_order_after) is one piece: its copy runs
    // under the kernels of the batch before it, on the other context.
    c->host_feed = getenv("FID_NO_FEED_OVERLAP") == nullptr;
    c->piece_chain = false;  // (frames that come up from the host are cut by the copy's pieces)
    const SubPlan plan = plan_sub_batches(c, nframes);
    const int nsub = plan.nsub;
    if (c->blocking && nsub == 1 && !c->wait_ev && !c->wait_copy_ev) {
        // one piece, nothing to overlap with: the copy goes on the main stream itself (no event between it and the first kernel)
        // BEHIND the clear of the result block, which so runs under the copy instead of after it (the single-frame call: 34 us
        // between the end of the copy and the start of the threshold kernel, round 4 timeline)
        c->host_feed = false;
        layout_results(c, nframes);
        HIPCHK(c, hipMemsetAsync(c->d_res, 0, c->res_clear_bytes, c->stream));
        c->res_precleared = true;
    }
    if (c->host_feed && !c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (c->host_feed && c->wait_copy_ev) HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->wait_copy_ev, 0));
    c->wait_copy_ev = nullptr;
    if (!c->host_feed) {
        HIPCHK(c, hipMemcpyAsync(c->in.data(), imgs, need, hipMemcpyHostToDevice, c->stream));
    } else {
        // (the copy stream must not overtake the previous call's kernels that still read d_in: they were synchronised at its end)
        for (int sb = 0; sb < nsub; sb++) {
            const int f0 = plan.f0[sb], Fs = plan.f0[sb + 1] - f0;
            const size_t off = (size_t)frame_stride * f0;
            const size_t bytes = (size_t)frame_stride * (Fs - 1) + (size_t)stride * height;
            HIPCHK(c, hipMemcpyAsync(c->in.data() + off, imgs + off, bytes, hipMemcpyHostToDevice, c->copy_stream));
            HIPCHK(c, hipEventRecord(c->in_ready[sb], c->copy_stream));
        }
    }
    const bool fed = c->host_feed;
    c->from_host_call = true;  // (enqueue_detect plans the same sub-batches: no piece chain, FID_NO_FEED_OVERLAP or not)
    const fid_status rc = enqueue_detect(c, c->in.data(), nframes, width, height, stride, frame_stride, enc);
    c->host_feed = c->from_host_call = false;
    if (rc == FID_OK) {
        c->fed_from_host = fed;
    } else {
        // (a HIP error half way through the enqueue: nothing will ever wait for the copies, so wait for them here -- the caller's
        //  buffer is not read after this function has returned an error)
        if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamSynchronize(c->stream);
        c->wait_ev = c->wait_copy_ev = nullptr;
        c->chained = false;
    }
    return rc;
}

fid_status fid_detect_batch(fid_ctx *c, const uint8_t *imgs, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                            int64_t frame_stride, fid_encoding enc, fid_marker *out, int32_t cap_per_frame, int32_t *n_per_frame)
{
    if (!out || !n_per_frame || cap_per_frame < 0) return FID_E_INVALID_ARG;
    if (c) c->blocking = true;
    const fid_status rc = feed_and_enqueue(c, imgs, nframes, width, height, stride, frame_stride, enc);
    if (c) c->blocking = c->res_precleared = false;
    if (rc != FID_OK) return rc;
    return finish_detect(c, out, cap_per_frame, n_per_frame);
}

fid_status fid_submit_batch(fid_ctx *c, const uint8_t *imgs, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                            int64_t frame_stride, fid_encoding enc)
{
    const fid_status rc = feed_and_enqueue(c, imgs, nframes, width, height, stride, frame_stride, enc);
    if (c) {
        c->wait_ev = nullptr;
        c->wait_copy_ev = nullptr;
        c->chained = false;
    }
    return rc;
}

fid_status fid_detect(fid_ctx *c, const uint8_t *img, int32_t width, int32_t height, int32_t stride, fid_encoding enc,
                      fid_marker *out, int32_t cap, int32_t *n)
{
    return fid_detect_batch(c, img, 1, width, height, stride, (int64_t)stride * height, enc, out, cap, n);
}

// k_pose (+ k_pose_cov) on the context's stream, timed as the pose stage
static fid_status run_pose(fid_ctx *c, const fid_marker *d_markers, const int *d_n, int n_stride_ints, const double *d_lens, int F, int per_frame,
                           const PoseAsk &a, fid_pose_out *d_out, fid_pose_cov *d_cov)
{
    pose_launch(c, c->stream, c->pose_ev[0], c->pose_ev[1], d_markers, d_n, n_stride_ints, d_lens, F, per_frame, a, d_out, d_cov);
    HIPCHK(c, hipGetLastError());
    return FID_OK;
}

fid_status fid_pose_last(fid_ctx *c, const double K[9], const double D[5], double fiducial_len, fid_pose_out *out,
                         int32_t cap_per_frame)
{
    if (!K) return FID_E_INVALID_ARG;
    const fid_camera cam = fid_camera_plumb_bob(K, D);
    return fid_pose_last_cam(c, &cam, fiducial_len, out, cap_per_frame);
}

// a fid_pose_cov beside every fid_pose_out of a call of the context's largest batch, on the device (the first _cov call allocates it:
// max_batch x max_markers_per_frame x 592 bytes, 39 MB at 256 x 256).  The records stay there; a _cov call copies out what the
// frames' counts need
static fid_status ensure_pose_cov(fid_ctx *c)
{
    const size_t need = (size_t)c->lim.max_batch * (size_t)c->lim.max_markers_per_frame;
    if (c->pcov.cap() >= need) return FID_OK;
    HIPCHK(c, c->pcov.reserve(need));
    HIPCHK(c, hipMemsetAsync(c->pcov.data(), 0, sizeof(fid_pose_cov) * need, c->stream));
    return FID_OK;
}

// fid_pose_last_cam and fid_pose_last_cov_cam: the poses (with_cov: and their covariances) of the last call's markers
static fid_status pose_last_run(fid_ctx *c, const fid_camera *camera, double fiducial_len, fid_pose_out *out, int32_t cap_per_frame, bool with_cov,
                                double sigma_px, fid_pose_cov *cov)
{
    if (!c || !fid_camera_usable(camera) || !out || c->last_frames <= 0 || !(fiducial_len > 0)) return FID_E_INVALID_ARG;
    if (with_cov && (!cov || !fid_sigma_usable(sigma_px))) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int F = c->last_frames, MM = c->P.maxMarkers;
    const PoseAsk ask = {fid_camera_normalised(*camera), fiducial_len, with_cov, sigma_px, {}};
    fid_status rc = with_cov ? ensure_pose_cov(c) : FID_OK;
    if (rc != FID_OK) return rc;
    if (!c->pose_req.answers(ask)) {  // (else the detect call already ran k_pose -- and k_pose_cov -- for this camera on these markers)
        rc = run_pose(c, c->d_markers, &c->d_counts[0].nmark, (int)(sizeof(DevCounts) / sizeof(int)), nullptr, F, MM, ask, c->d_poses, c->pcov.data());
        if (rc != FID_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(c->h_poses, c->d_poses, sizeof(fid_pose_out) * (size_t)F * MM, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->profile) (void)hipEventElapsedTime(&c->stage_ms[ST_POSE], c->pose_ev[0], c->pose_ev[1]);
        c->pose_req.answered(ask);  // (asked for without its covariance: the next call runs k_pose alone)
    }
    int nmax = 0;
    for (int f = 0; f < F; f++) {
        int n = c->h_counts[f].nmark;
        if (n > cap_per_frame) {
            n = cap_per_frame;
            rc = FID_E_CAPACITY;
        }
        nmax = n > nmax ? n : nmax;
        memcpy(out + (size_t)f * cap_per_frame, c->h_poses + (size_t)f * MM, sizeof(fid_pose_out) * n);
    }
    if (with_cov && nmax > 0) {
        // the first nmax records of every frame in one strided copy, straight into the caller's array (a frame with fewer markers
        // gets records beyond its count along: they are not part of the result)
        HIPCHK(c, hipMemcpy2DAsync(cov, sizeof(fid_pose_cov) * (size_t)cap_per_frame, c->pcov.data(), sizeof(fid_pose_cov) * (size_t)MM,
                                   sizeof(fid_pose_cov) * (size_t)nmax, (size_t)F, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return rc;
}

fid_status fid_pose_last_cam(fid_ctx *c, const fid_camera *camera, double fiducial_len, fid_pose_out *out, int32_t cap_per_frame)
{
    return pose_last_run(c, camera, fiducial_len, out, cap_per_frame, false, 0., nullptr);
}

fid_status fid_pose_last_cov_cam(fid_ctx *c, const fid_camera *camera, double fiducial_len, fid_pose_out *out, int32_t cap_per_frame,
                                 double sigma_px, fid_pose_cov *cov)
{
    return pose_last_run(c, camera, fiducial_len, out, cap_per_frame, true, sigma_px, cov);
}

fid_status fid_pose(fid_ctx *c, const double K[9], const double D[5], const fid_marker *markers, const double *len_per_marker,
                    int32_t n, double fiducial_len, fid_pose_out *out)
{
    if (!K) return FID_E_INVALID_ARG;
    const fid_camera cam = fid_camera_plumb_bob(K, D);
    return fid_pose_cam(c, &cam, markers, len_per_marker, n, fiducial_len, out);
}

static fid_status pose_cam_run(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, const double *len_per_marker, int32_t n,
                               double fiducial_len, fid_pose_out *out, bool with_cov, double sigma_px, fid_pose_cov *cov)
{
    if (!c || !fid_camera_usable(camera) || (n > 0 && (!markers || !out)) || n < 0 || !(fiducial_len > 0)) return FID_E_INVALID_ARG;
    if (n == 0) return FID_OK;
    if (len_per_marker)
        for (int i = 0; i < n; i++)
            if (!(len_per_marker[i] > 0)) return FID_E_INVALID_ARG;  // CV_Assert(markerLength > 0), aruco_detect.cpp:229
    if (refuse_in_flight(c)) return FID_E_INVALID_ARG;  // (shares the context's stream and buffers with the batch in flight)
    HIPCHK(c, hipSetDevice(c->device));
    if (n > c->pose_cap) {
        const int cap = roundup(n, 256);
        MemLayout l;
        l.add(&c->d_pose_in, cap), l.add(&c->d_pose_out, cap), l.add(&c->d_lens, cap);
        c->pose_cap = 0;
        HIPCHK(c, c->pose_mem.reserve(l.bytes()));
        l.bind(c->pose_mem.p);
        c->pose_cap = cap;
    }
    fid_pose_out *d_out = c->d_pose_out;
    HIPCHK(c, hipMemcpyAsync(c->d_pose_in, markers, sizeof(fid_marker) * n, hipMemcpyHostToDevice, c->stream));
    std::vector<double> lens(n);
    for (int i = 0; i < n; i++) lens[i] = len_per_marker ? len_per_marker[i] : fiducial_len;
    HIPCHK(c, hipMemcpyAsync(c->d_lens, lens.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    int nn = n;
    HIPCHK(c, hipMemcpyAsync(c->d_pose_n, &nn, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // lens/nn are stack/heap temporaries
    if (with_cov) HIPCHK(c, c->pcov_in.reserve((size_t)n, (size_t)c->pose_cap));
    fid_status rc = run_pose(c, c->d_pose_in, c->d_pose_n, 0, c->d_lens, 1, n, {*camera, fiducial_len, with_cov, sigma_px, {}}, d_out, c->pcov_in.data());
    if (rc != FID_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(out, d_out, sizeof(fid_pose_out) * n, hipMemcpyDeviceToHost, c->stream));
    if (with_cov) HIPCHK(c, hipMemcpyAsync(cov, c->pcov_in.data(), sizeof(fid_pose_cov) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FID_OK;
}

fid_status fid_pose_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, const double *len_per_marker, int32_t n,
                        double fiducial_len, fid_pose_out *out)
{
    return pose_cam_run(c, camera, markers, len_per_marker, n, fiducial_len, out, false, 0., nullptr);
}

fid_status fid_pose_cov_cam(fid_ctx *c, const fid_camera *camera, const fid_marker *markers, const double *len_per_marker, int32_t n,
                            double fiducial_len, fid_pose_out *out, double sigma_px, fid_pose_cov *cov)
{
    if (!fid_sigma_usable(sigma_px) || (n > 0 && !cov)) return FID_E_INVALID_ARG;
    return pose_cam_run(c, camera, markers, len_per_marker, n, fiducial_len, out, true, sigma_px, cov);
}

fid_status fid_project_points_cam(fid_ctx *c, const fid_camera *camera, const double rvec[3], const double tvec[3], const double *obj_xyz,
                                  int32_t n, double *uv, double *jac)
{
    if (!c || !fid_camera_usable(camera) || !rvec || !tvec || n < 0 || (n > 0 && (!obj_xyz || !uv))) return FID_E_INVALID_ARG;
    if (n == 0) return FID_OK;
    if (refuse_in_flight(c)) return FID_E_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    // one block of device memory for the call: the points, the projections, the Jacobian rows (a utility, not a hot path)
    const size_t nn = (size_t)n;
    double *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, sizeof(double) * nn * (3 + 2 + 12)));
    double *d_obj = d, *d_uv = d + 3 * nn, *d_jac = d + 5 * nn;
    const PoseCam cam = pose_cam_from(*camera, 0.);
    PosePar par;
    for (int i = 0; i < 3; i++) {
        par.v[i] = rvec[i];
        par.v[3 + i] = tvec[i];
    }
    hipError_t e = hipMemcpyAsync(d_obj, obj_xyz, sizeof(double) * 3 * nn, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        POSE_CAM_DISPATCH(cam.model, hipLaunchKernelGGL(k_project_points<CAM_MODEL>, dim3((unsigned)((2 * nn + 63) / 64)), dim3(64), 0, c->stream, cam, par,
                                                        (const double *)d_obj, (int)n, d_uv, jac ? d_jac : (double *)nullptr));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(uv, d_uv, sizeof(double) * 2 * nn, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && jac) e = hipMemcpyAsync(jac, d_jac, sizeof(double) * 12 * nn, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCHK(c, e);
    return FID_OK;
}

// sensor_msgs/CameraInfo -> fid_camera (fid_abi.h has the table).  Host code.
static thread_local std::string g_camera_error;
const char *fid_camera_last_error(void) { return g_camera_error.c_str(); }
fid_status fid_camera_from_info(const char *distortion_model, const double K[9], const double *D, int32_t n_D, fid_camera *out)
{
    g_camera_error.clear();
    if (!distortion_model || !K || !out || n_D < 0 || (n_D > 0 && !D)) {
        g_camera_error = "camera: a NULL pointer or a negative coefficient count";
        return FID_E_INVALID_ARG;
    }
    const std::string m(distortion_model);
    const std::string given = "distortion_model \"" + m + "\" with " + std::to_string(n_D) + " coefficients";
    int model = -1, n_dist = 0;
    if (m.empty() || m == "plumb_bob") {
        if (n_D == 4 || n_D == 5) model = FID_CAM_PLUMB_BOB, n_dist = n_D;
    } else if (m == "rational_polynomial") {
        if (n_D == 8 || n_D == 12) model = FID_CAM_RATIONAL, n_dist = n_D;
        if (n_D == 14) {
            if (D[12] == 0. && D[13] == 0.) {
                model = FID_CAM_RATIONAL, n_dist = 12;
            } else if (D[12] - D[12] == 0. && D[13] - D[13] == 0.) {
                g_camera_error = "camera: " + given + " has a tilted sensor (taux = " + std::to_string(D[12]) + ", tauy = " + std::to_string(D[13]) +
                                 "), which is not supported";
                return FID_E_UNSUPPORTED;
            }
        }
    } else if (m == "equidistant" || m == "fisheye") {
        if (n_D == 4) model = FID_CAM_EQUIDISTANT, n_dist = 4;
    }
    bool finite = true;
    for (int i = 0; i < 9; i++) finite = finite && K[i] - K[i] == 0.;
    for (int i = 0; i < n_D; i++) finite = finite && D[i] - D[i] == 0.;
    if (!finite) {
        g_camera_error = "camera: K or D holds a value that is not finite";
        return FID_E_INVALID_ARG;
    }
    if (model < 0) {
        g_camera_error = "camera: " + given + " is not supported (plumb_bob: 4 or 5, rational_polynomial: 8, 12 or 14 with zero tilt, equidistant / fisheye: 4)";
        return FID_E_UNSUPPORTED;
    }
    if (K[0] == 0. || K[4] == 0.) {
        g_camera_error = "camera: fx and fy must not be zero";
        return FID_E_INVALID_ARG;
    }
    fid_camera cam;
    cam.model = model;
    cam.n_dist = n_dist;
    for (int i = 0; i < 9; i++) cam.K[i] = K[i];
    for (int i = 0; i < 12; i++) cam.D[i] = i < n_dist ? D[i] : 0.;
    *out = cam;
    return FID_OK;
}

fid_status fid_refine_contour_corners(fid_ctx *c, const int32_t *pts_xy, const int32_t *offsets, int32_t n, float *corners,
                                      int32_t *status_per_marker)
{
    if (!c || !pts_xy || !offsets || !corners || !status_per_marker || n < 0) return FID_E_INVALID_ARG;
    if (refuse_in_flight(c)) return FID_E_INVALID_ARG;
    if (n == 0) return FID_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (offsets[0] != 0) return FID_E_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return FID_E_INVALID_ARG;
    const int total = offsets[n];
    std::vector<uint32_t> packed((size_t)(total > 0 ? total : 1));
    for (int k = 0; k < total; k++) {
        const int x = pts_xy[2 * k], y = pts_xy[2 * k + 1];
        if (x < 0 || y < 0 || x > 0xffff || y > 0xffff) return FID_E_INVALID_ARG;
        packed[k] = (uint32_t)x | ((uint32_t)y << 16);
    }
    uint32_t *d_pts = nullptr;
    int *d_off = nullptr, *d_status = nullptr;
    float *d_corners = nullptr;
    fid_status rc = FID_OK;
    auto chk = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == FID_OK) {
            c->last_error = std::string(what) + ": " + hipGetErrorString(e);
            rc = e == hipErrorOutOfMemory ? FID_E_OUT_OF_MEMORY : FID_E_HIP;
        }
    };
    chk(hipMalloc((void **)&d_pts, packed.size() * sizeof(uint32_t)), "hipMalloc");
    chk(hipMalloc((void **)&d_off, (size_t)(n + 1) * sizeof(int)), "hipMalloc");
    chk(hipMalloc((void **)&d_status, (size_t)n * sizeof(int)), "hipMalloc");
    chk(hipMalloc((void **)&d_corners, (size_t)n * 8 * sizeof(float)), "hipMalloc");
    if (rc == FID_OK) {
        chk(hipMemcpyAsync(d_pts, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
        chk(hipMemcpyAsync(d_off, offsets, (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
        chk(hipMemcpyAsync(d_corners, corners, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
    }
    if (rc == FID_OK) {
        hipLaunchKernelGGL(k_refine_contour_pts, dim3(n), dim3(64), 0, c->stream, (const uint32_t *)d_pts, (const int *)d_off, d_corners, d_status);
        chk(hipGetLastError(), "k_refine_contour_pts");
        chk(hipMemcpyAsync(corners, d_corners, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
        chk(hipMemcpyAsync(status_per_marker, d_status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
        chk(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    }
    (void)hipFree(d_pts);
    (void)hipFree(d_off);
    (void)hipFree(d_status);
    (void)hipFree(d_corners);
    if (rc == FID_OK)
        for (int i = 0; i < n; i++)
            if (status_per_marker[i]) rc = FID_E_CV_EXCEPTION;
    return rc;
}

int64_t fid_tap_bytes(fid_ctx *c, fid_tap which)
{
    if (!c || c->last_frames <= 0) return 0;
    const DevParams &P = c->P;
    const int64_t F = c->last_frames;
    const int msb = P.markerSize + 2 * P.borderBits;
    switch (which) {
    case FID_TAP_MASKS: return F * P.nscales * P.H * P.WW * 4;
    case FID_TAP_CANDIDATES:
    case FID_TAP_FILTERED: return F * P.maxCands * (int64_t)sizeof(fid_candidate);
    case FID_TAP_BITS: return F * P.maxCands * msb * msb;
    case FID_TAP_IDENT: return F * P.maxCands * 8;
    case FID_TAP_PRESUBPIX: return F * P.maxMarkers * (int64_t)sizeof(fid_marker);
    case FID_TAP_COUNTS: return F * 12 * 4;
    case FID_TAP_GRAY: return F * (int64_t)P.W * P.H;
    }
    return 0;
}

fid_status fid_tap_read(fid_ctx *c, fid_tap which, void *dst, int64_t dst_bytes)
{
    if (!c || !dst || c->last_frames <= 0 || c->in_flight) return FID_E_INVALID_ARG;
    int64_t need = fid_tap_bytes(c, which);
    if (need <= 0 || dst_bytes < need) return FID_E_CAPACITY;
    HIPCHK(c, hipSetDevice(c->device));
    const DevParams &P = c->P;
    const int F = c->last_frames;
    const int msb = P.markerSize + 2 * P.borderBits;
    switch (which) {
    case FID_TAP_MASKS: {
        // un-tile on the host
        const size_t plane = (size_t)P.TR * P.TC * MT_ROWS;
        std::vector<uint32_t> tmp(plane);
        for (int fs = 0; fs < F * P.nscales; fs++) {
            HIPCHK(c, hipMemcpy(tmp.data(), c->d_masks + (size_t)fs * plane, plane * 4, hipMemcpyDeviceToHost));
            uint32_t *o = (uint32_t *)dst + (size_t)fs * P.H * P.WW;
            for (int y = 0; y < P.H; y++)
                for (int w = 0; w < P.WW; w++) o[(size_t)y * P.WW + w] = tmp[(size_t)mask_word(P.TC, y + 1, MASK_PADW + w)];
        }
        return FID_OK;
    }
    case FID_TAP_CANDIDATES:
    case FID_TAP_FILTERED: {
        std::vector<DevCand> tmp((size_t)F * P.maxCands);
        HIPCHK(c, hipMemcpy(tmp.data(), which == FID_TAP_CANDIDATES ? c->d_sorted : c->d_filtered, tmp.size() * sizeof(DevCand),
                            hipMemcpyDeviceToHost));
        fid_candidate *o = (fid_candidate *)dst;
        for (size_t i = 0; i < tmp.size(); i++) {
            o[i].scale = tmp[i].scale;
            o[i].contour_size = tmp[i].size;
            o[i].start_x = tmp[i].sx;
            o[i].start_y = tmp[i].sy;
            o[i].is_hole = tmp[i].hole;
            memcpy(o[i].corners, tmp[i].c, sizeof(float) * 8);
        }
        return FID_OK;
    }
    case FID_TAP_BITS:
        HIPCHK(c, hipMemcpy(dst, c->d_bits, (size_t)F * P.maxCands * msb * msb, hipMemcpyDeviceToHost));
        return FID_OK;
    case FID_TAP_IDENT: {
        std::vector<DevIdent> tmp((size_t)F * P.maxCands);
        HIPCHK(c, hipMemcpy(tmp.data(), c->d_ident, tmp.size() * sizeof(DevIdent), hipMemcpyDeviceToHost));
        int32_t *o = (int32_t *)dst;
        for (size_t i = 0; i < tmp.size(); i++) {
            o[2 * i] = tmp[i].id;
            o[2 * i + 1] = tmp[i].rot;
        }
        return FID_OK;
    }
    case FID_TAP_PRESUBPIX:
        HIPCHK(c, hipMemcpy(dst, c->d_pre, (size_t)need, hipMemcpyDeviceToHost));
        return FID_OK;
    case FID_TAP_COUNTS: {
        int32_t *o = (int32_t *)dst;
        for (int f = 0; f < F; f++) {
            o[12 * f + 0] = c->h_counts[f].nstarts;
            o[12 * f + 1] = c->whole_border_walk ? (c->h_counts[f].nsurv < c->P.maxContours ? c->h_counts[f].nsurv : c->P.maxContours) : c->h_counts[f].ncontours + c->h_counts[f].ncontours2;
            o[12 * f + 10] = c->h_counts[f].nseeds;
            o[12 * f + 2] = c->h_counts[f].ncand;
            o[12 * f + 3] = c->h_counts[f].nfilt;
            o[12 * f + 4] = c->h_counts[f].nacc;
            o[12 * f + 5] = c->h_counts[f].nmark;
            o[12 * f + 6] = c->h_counts[f].overflow | ((int32_t)c->h_global->overflow << 8);
            o[12 * f + 7] = c->h_counts[f].nsurv;
            // (cycle tracing: per frame, from the walks' lengths; the whole-border walk has only the allocator's head, in whole arenas)
            o[12 * f + 8] = c->whole_border_walk ? c->h_counts[f].npool : c->h_counts[f].nchunks;
            o[12 * f + 9] = c->h_counts[f].nsurv1;
            o[12 * f + 11] = c->h_counts[f].ndense;  // contour points handed to approxPolyDP (every contour's rounded up to 8)
        }
        return FID_OK;
    }
    case FID_TAP_GRAY:
        for (int f = 0; f < F; f++)
            HIPCHK(c, hipMemcpy2D((char *)dst + (size_t)f * P.W * P.H, (size_t)P.W, c->last_gray + (size_t)f * c->last_gfstride,
                                  (size_t)P.gstride, (size_t)P.W, P.H, hipMemcpyDeviceToHost));
        return FID_OK;
    }
    return FID_E_INVALID_ARG;
}

int32_t fid_last_stage_ms(fid_ctx *c, float *ms, int32_t cap, const char *const **names)
{
    if (names) *names = kStageNames;
    if (!c || !ms) return ST_COUNT;
    for (int i = 0; i < ST_COUNT && i < cap; i++) ms[i] = c->profile ? c->stage_ms[i] : -1.f;
    return ST_COUNT;
}

int32_t fid_last_launches(fid_ctx *c) { return c ? c->last_nsub : 0; }

void *fid_stream(fid_ctx *c) { return c ? (void *)c->stream : nullptr; }

const char *fid_strerror(fid_status s)
{
    switch (s) {
    case FID_OK: return "ok";
    case FID_E_INVALID_ARG: return "invalid argument";
    case FID_E_NO_DEVICE: return "no HIP device (this library has no CPU fallback)";
    case FID_E_HIP: return "HIP runtime error";
    case FID_E_CAPACITY: return "capacity exceeded";
    case FID_E_OUT_OF_MEMORY: return "out of memory";
    case FID_E_CV_EXCEPTION:
        return "the reference's OpenCV call throws cv::Exception on this input (n = -1 for the frame)";
    case FID_E_UNSUPPORTED: return "unsupported parameter combination";
    }
    return "unknown status";
}

const char *fid_last_error(fid_ctx *c) { return c ? c->last_error.c_str() : ""; }

int32_t fid_abi_version(void) { return FID_ABI_VERSION; }

}  // extern "C"

#include "fid_stag.hip"
#include "fid_jpeg.hip"
#include "fid_png.hip"
#include "fid_draw.hip"
#include "fid_jpeg_enc.hip"
#include "fid_dict.hip"
#include "fid_stag_layout.hip"
#include "fid_map.hip"
#include "fid_map_pose.hip"
#include "fid_map_pose_robust.hip"
#include "fid_calib.hip"
#include "fid_map_build.hip"
#include "fid_charuco.hip"
#include "fid_calib_points.hip"
#include "fid_diamond.hip"
#include "fid_rig_pose.hip"
