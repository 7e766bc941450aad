// JPEG encoding on the device -- included by fid_api.hip (one translation unit), behind fid_draw.hip.
//
// The way out of the compressed road: image_transport offers <topic>/compressed for every image publisher (the node's
// /fiducial_images among them, aruco_detect.cpp:662), and its compressed publisher makes that message with
// cv::imencode(".jpg", bgr, {IMWRITE_JPEG_QUALITY, q}) = libjpeg(-turbo) with its defaults: baseline sequential DCT, 8 bit,
// JDCT_ISLOW, the Annex K Huffman tables (no optimised tables), no restart markers, three components in one interleaved scan or one
// component alone.  The kernels here write that file, byte for byte (tests/jpeg_encode_restatement.py is the same arithmetic in
// numpy, pinned on libjpeg-turbo's own files), for a batch of frames that lie in HBM, in seven launches with the frames as a grid
// dimension:
//   1 k_jenc_dct      colour conversion (jccolor.c rgb_ycc_convert), chroma downsampling with edge replication (jcsample.c,
//                     jcprepct.c) fused into the load, jpeg_fdct_islow (jfdctint.c) and quantisation (jcdctmgr.c): 8 lanes a block,
//                     a row, then a column per lane, the transpose through LDS.  The frame is read, the planes are never written.
//   2 k_jenc_len      a lane per block in SCAN order: the bits the block codes to (jchuff.c encode_one_block).  The DC difference
//                     needs the block coded before it of the same component, which another lane of (1) makes: hence a pass of
//                     its own.  Dummy blocks (jccoefct.c compress_data) get the DC of the block in front of them here.
//   3 k_jenc_scan     exclusive scan of the lengths per frame = every block's bit offset; clears the words the scan will occupy
//                     and sets the 1-bits that pad the last byte.
//   4 k_jenc_emit     a lane per block again: the code words, shifted to the block's offset, as whole 32-bit words -- plain stores for
//                     the words a block owns, atomicOr into the cleared word for the one or two it shares with its neighbours.
//   5 k_jenc_ffcount  0xFF bytes per tile of the bit stream,
//   6 k_jenc_ffscan   their exclusive scan per frame = where every tile lands in the file; the file's length,
//   7 k_jenc_pack     header, every byte at its final place with 0x00 behind each 0xFF, FF D9.
// Worst case, for sizing: a block codes to at most 11 + 11 bits of DC (the longest DC code, the largest size category) and 63 x (16
// + 10) bits of AC (the longest AC code, category 10) = 1660 bits = 207.5 bytes for its 64 samples; stuffing at most doubles that:
// 415 bytes a block, 6.5 bytes a sample, against the 0.1 - 0.3 a camera frame takes.  A context therefore does NOT reserve the
// worst case per frame: max_file_bytes bounds a file, a frame that does not fit is refused (FID_E_CAPACITY, with the size it
// needs), and never comes back cut short.

#define JE_TPB 256
#define JE_DCT_BLOCKS 32      // 8 x 8 blocks a workgroup of k_jenc_dct transforms (8 lanes each)
#define JE_SCAN_TPB 1024
#define JE_SCAN_PER 4         // items per lane: k_jenc_scan / k_jenc_ffscan take JE_SCAN_TPB * JE_SCAN_PER = 4096 items a round
#define JE_STUFF_TILE 4096    // bytes of the bit stream per tile of k_jenc_ffcount / k_jenc_pack (16 per lane)
#define JE_HDR_MAX 640        // 623 bytes for three components, 328 for one
#define JE_OVER_BITS 1u       // JeFrame.flags: the entropy-coded bytes do not fit the bit buffer
#define JE_OVER_FILE 2u       //                the file does not fit max_file_bytes

struct JeGeom {
    int W, H, ncomp, hs, vs, mcux, mcuy, bpm;  // bpm: blocks per MCU
    int rw[3], rh[3];                          // blocks that hold samples (width_in_blocks, height_in_blocks)
    int sw[3], sh[3];                          // blocks in the scan = in the tap: MCU-padded for three components
    int cbase[3];                              // first block of a component in the tap layout
    int nblk;                                  // blocks per frame
    int enc, stride, hdr_len;
    long long fstride;
};
struct JeTables {
    uint32_t dc[2][16];    // length << 16 | code by size category
    uint32_t ac[2][256];   // ... by run << 4 | size
    uint32_t q8[2][64];    // 8 x quantiser, natural order (jpeg_fdct_islow leaves its output scaled by 8)
    uint32_t qm[2][64];    // floor(2^32 / q8) + 1: n / q8 == umulhi(n, qm) for every n the transform can give (n x q8 < 2^32)
    uint8_t hdr[JE_HDR_MAX];
};
struct JeFrame {
    unsigned long long bits;    // entropy-coded bits
    unsigned long long nbytes;  // the file
    uint32_t nff, flags;
};

namespace {

const uint8_t kJeStdLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kJeStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// ITU-T T.81 Annex K.3 (jcparam.c std_huff_tables): BITS, HUFFVAL
const uint8_t kJeDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kJeDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kJeAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kJeAcVals[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// jpeg_quality_scaling + jpeg_add_quant_table(force_baseline = TRUE): natural order
void je_quant_table(const uint8_t *std_tbl, int quality, uint32_t *out)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; i++) {
        int v = ((int)std_tbl[i] * scale + 50) / 100;
        out[i] = (uint32_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

// jpeg_make_c_derived_tbl: length << 16 | code by symbol
void je_derive(const uint8_t *bits, const uint8_t *vals, uint32_t *out, int nout)
{
    for (int i = 0; i < nout; i++) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = (uint32_t)len << 16 | code++;
        code <<= 1;
    }
}

void je_sampling(int subsampling, int components, int *hs, int *vs)
{
    *hs = components == 3 && subsampling >= 1 ? 2 : 1;
    *vs = components == 3 && subsampling == 2 ? 2 : 1;
}

// every byte in front of the entropy-coded data (jcmarker.c: write_file_header, write_frame_header, write_scan_header); out holds
// JE_HDR_MAX bytes
int je_header(int quality, int subsampling, int W, int H, int ncomp, uint8_t *out)
{
    int n = 0;
    auto put = [&](int v) { out[n++] = (uint8_t)v; };
    auto seg = [&](int marker, int body) {
        put(0xFF);
        put(marker);
        put((body + 2) >> 8);
        put((body + 2) & 255);
    };
    put(0xFF);
    put(0xD8);
    seg(0xE0, 14);  // JFIF 1.01, no units, density 1 x 1, no thumbnail
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (uint8_t b : jfif) put(b);
    for (int t = 0; t < (ncomp == 3 ? 2 : 1); t++) {
        uint32_t q[64];
        je_quant_table(t ? kJeStdChroma : kJeStdLuma, quality, q);
        seg(0xDB, 65);
        put(t);
        for (int k = 0; k < 64; k++) put((int)q[kJpZigzag[k]]);
    }
    int hs, vs;
    je_sampling(subsampling, ncomp, &hs, &vs);
    seg(0xC0, 6 + 3 * ncomp);
    put(8);
    put(H >> 8);
    put(H & 255);
    put(W >> 8);
    put(W & 255);
    put(ncomp);
    for (int c = 0; c < ncomp; c++) {
        put(c + 1);
        put(c == 0 ? (hs << 4 | vs) : 0x11);
        put(c == 0 ? 0 : 1);
    }
    for (int t = 0; t < (ncomp == 3 ? 2 : 1); t++) {
        seg(0xC4, 1 + 16 + 12);
        put(t);
        for (int i = 0; i < 16; i++) put(kJeDcBits[t][i]);
        for (int i = 0; i < 12; i++) put(kJeDcVals[i]);
        seg(0xC4, 1 + 16 + 162);
        put(0x10 | t);
        for (int i = 0; i < 16; i++) put(kJeAcBits[t][i]);
        for (int i = 0; i < 162; i++) put(kJeAcVals[t][i]);
    }
    seg(0xDA, 4 + 2 * ncomp);
    put(ncomp);
    for (int c = 0; c < ncomp; c++) {
        put(c + 1);
        put(c == 0 ? 0x00 : 0x11);
    }
    put(0);
    put(63);
    put(0);
    return n;
}

void je_geometry(int W, int H, int ncomp, int subsampling, JeGeom *G)
{
    memset(G, 0, sizeof(*G));
    G->W = W;
    G->H = H;
    G->ncomp = ncomp;
    je_sampling(subsampling, ncomp, &G->hs, &G->vs);
    if (ncomp == 1) {  // a scan of one component: its MCU is one block, there are no dummy blocks
        G->mcux = (W + 7) / 8;
        G->mcuy = (H + 7) / 8;
        G->bpm = 1;
        G->rw[0] = G->sw[0] = G->mcux;
        G->rh[0] = G->sh[0] = G->mcuy;
    } else {
        G->mcux = (W + 8 * G->hs - 1) / (8 * G->hs);
        G->mcuy = (H + 8 * G->vs - 1) / (8 * G->vs);
        G->bpm = G->hs * G->vs + 2;
        G->rw[0] = (W + 7) / 8;
        G->rh[0] = (H + 7) / 8;
        G->sw[0] = G->mcux * G->hs;
        G->sh[0] = G->mcuy * G->vs;
        const int cw = (W + G->hs - 1) / G->hs, ch = (H + G->vs - 1) / G->vs;
        for (int c = 1; c < 3; c++) {
            G->rw[c] = (cw + 7) / 8;
            G->rh[c] = (ch + 7) / 8;
            G->sw[c] = G->mcux;
            G->sh[c] = G->mcuy;
        }
    }
    int at = 0;
    for (int c = 0; c < ncomp; c++) {
        G->cbase[c] = at;
        at += G->sw[c] * G->sh[c];
    }
    G->nblk = at;
}

// ---------------------------------------------------------------- 1: samples -> quantised coefficients

// one component of one pixel (jccolor.c rgb_ycc_convert: 16-bit fixed point; Cb and Cr round with ONE_HALF - 1)
__device__ __forceinline__ int je_component(const uint8_t *p, int enc, int c)
{
    if (enc == FID_ENC_MONO8) return p[0];
    const int r = enc == FID_ENC_RGB8 ? p[0] : p[2], g = p[1], b = enc == FID_ENC_RGB8 ? p[2] : p[0];
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// one pass of jpeg_fdct_islow over eight values (13-bit constants, PASS1_BITS = 2; FIRST: the row pass)
template <bool FIRST>
__device__ __forceinline__ void je_fdct8(int (&d)[8])
{
    constexpr int N = FIRST ? JP_CONST_BITS - JP_PASS1_BITS : JP_CONST_BITS + JP_PASS1_BITS, R = 1 << (N - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << JP_PASS1_BITS;
        d[4] = (t10 - t11) << JP_PASS1_BITS;
    } else {
        d[0] = (t10 + t11 + (1 << (JP_PASS1_BITS - 1))) >> JP_PASS1_BITS;
        d[4] = (t10 - t11 + (1 << (JP_PASS1_BITS - 1))) >> JP_PASS1_BITS;
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = (z1 + t13 * 6270 + R) >> N;
    d[6] = (z1 - t12 * 15137 + R) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = (m4 + z1 + z3 + R) >> N;
    d[5] = (m5 + z2 + z4 + R) >> N;
    d[3] = (m6 + z2 + z3 + R) >> N;
    d[1] = (m7 + z1 + z4 + R) >> N;
}

// coef: [frame][G.nblk][64] int16, component after component, [sh][sw] blocks each (the layout of FID_JPEG_TAP_COEFS)
__global__ __launch_bounds__(JE_TPB) void k_jenc_dct(const uint8_t *__restrict__ src, int16_t *__restrict__ coef, long long coef_fstride,
                                                      const JeTables *__restrict__ tab, const JeGeom G)
{
    __shared__ int s_t[JE_DCT_BLOCKS][65];
    const int tid = threadIdx.x, b = tid >> 3, r = tid & 7;
    const int blk = blockIdx.x * JE_DCT_BLOCKS + b;
    const bool live = blk < G.nblk;
    const int c = !live ? 0 : (G.ncomp == 3 && blk >= G.cbase[2] ? 2 : (G.ncomp == 3 && blk >= G.cbase[1] ? 1 : 0));
    const int sw = c == 0 ? G.sw[0] : G.sw[1], rw = c == 0 ? G.rw[0] : G.rw[1], rh = c == 0 ? G.rh[0] : G.rh[1];
    const int rel = blk - (c == 0 ? 0 : (c == 1 ? G.cbase[1] : G.cbase[2]));
    const int by = rel / sw, bx = rel - by * sw;
    int d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live && by < rh && bx < rw) {  // (a dummy block stays zero; k_jenc_len gives it its DC)
        const uint8_t *frame = src + (long long)blockIdx.y * G.fstride;
        const int bpp = G.enc == FID_ENC_MONO8 ? 1 : 3;
        const int hx = c == 0 ? 1 : G.hs, vy = c == 0 ? 1 : G.vs;
        // the sampled rows are replicated below the component's last row, the input rows below the image's
        const int ch = (G.H + vy - 1) / vy;
        const int cy = min(by * 8 + r, ch - 1);
        const uint8_t *row0 = frame + (long long)min(cy * vy, G.H - 1) * G.stride;
        const uint8_t *row1 = frame + (long long)min(cy * vy + vy - 1, G.H - 1) * G.stride;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int cx = bx * 8 + j;
            const int x0 = min(cx * hx, G.W - 1) * bpp, x1 = min(cx * hx + hx - 1, G.W - 1) * bpp;  // (the input's right edge replicated)
            int v;
            if (hx == 1)
                v = je_component(row0 + x0, G.enc, c);
            else if (vy == 1)  // h2v1_downsample: bias 0, 1, 0, 1, ...
                v = (je_component(row0 + x0, G.enc, c) + je_component(row0 + x1, G.enc, c) + (j & 1)) >> 1;
            else  // h2v2_downsample: bias 1, 2, 1, 2, ...
                v = (je_component(row0 + x0, G.enc, c) + je_component(row0 + x1, G.enc, c) + je_component(row1 + x0, G.enc, c) +
                     je_component(row1 + x1, G.enc, c) + 1 + (j & 1)) >> 2;
            d[j] = v - 128;
        }
    }
    je_fdct8<true>(d);
#pragma unroll
    for (int j = 0; j < 8; j++) s_t[b][r * 8 + j] = d[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; j++) d[j] = s_t[b][j * 8 + r];
    je_fdct8<false>(d);
    const int tq = c == 0 ? 0 : 1;
#pragma unroll
    for (int j = 0; j < 8; j++) {  // jcdctmgr.c quantize: (|v| + (q >> 1)) / q on the transform's 8-fold scale, the sign put back
        const int n = j * 8 + r;
        const uint32_t a = (uint32_t)abs(d[j]) + (tab->q8[tq][n] >> 1);
        const int qv = (int)__umulhi(a, tab->qm[tq][n]);
        s_t[b][n] = d[j] < 0 ? -qv : qv;  // (the lane's own eight places: nobody else reads them before the barrier)
    }
    __syncthreads();
    if (live) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) w[j] = (uint32_t)(s_t[b][r * 8 + 2 * j] & 0xffff) | (uint32_t)s_t[b][r * 8 + 2 * j + 1] << 16;
        *(uint4 *)(coef + (long long)blockIdx.y * coef_fstride + (long long)blk * 64 + r * 8) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---------------------------------------------------------------- 2 and 4: the entropy coder of one block

struct JeBlockAt {
    int c, by, bx;   // component, block row and column in the tap layout
    long long prev;  // tap index of the block whose DC this one is predicted from, -1 at the start of the scan
    long long self;  // tap index of this block
    long long from;  // a dummy block: the block that lends it its DC; else -1
};

// tap index of the i-th luma block of MCU m, or of the nearest block in front of it in the MCU that holds samples (block 0 always does)
__device__ __forceinline__ long long je_luma_source(const JeGeom &G, int m, int i)
{
    const int my = m / G.mcux, mx = m - my * G.mcux;
    for (;; i--) {
        const int by = my * G.vs + i / G.hs, bx = mx * G.hs + i % G.hs;
        if (i == 0 || (by < G.rh[0] && bx < G.rw[0])) return (long long)by * G.sw[0] + bx;
    }
}

// block s of the scan (MCU after MCU; inside an MCU the luma blocks row by row, then Cb, then Cr)
__device__ __forceinline__ JeBlockAt je_block_at(const JeGeom &G, int s)
{
    JeBlockAt a;
    const int m = s / G.bpm, i = s - m * G.bpm;
    const int my = m / G.mcux, mx = m - my * G.mcux;
    a.from = -1;
    if (G.ncomp == 1) {
        a.c = 0;
        a.by = my;
        a.bx = mx;
        a.self = s;
        a.prev = s - 1;
        return a;
    }
    const int nl = G.hs * G.vs;
    if (i < nl) {
        a.c = 0;
        a.by = my * G.vs + i / G.hs;
        a.bx = mx * G.hs + i % G.hs;
        a.self = (long long)a.by * G.sw[0] + a.bx;
        if (a.by >= G.rh[0] || a.bx >= G.rw[0]) a.from = je_luma_source(G, m, i - 1);
        a.prev = i > 0 ? je_luma_source(G, m, i - 1) : (m > 0 ? je_luma_source(G, m - 1, nl - 1) : -1);
    } else {
        a.c = i - nl + 1;
        a.by = my;
        a.bx = mx;
        a.self = G.cbase[a.c] + m;  // (sw == mcux for chroma: tap order is MCU order)
        a.prev = m > 0 ? a.self - 1 : -1;
    }
    return a;
}

// The bit stream as 32-bit words, most significant bit first.  A block starts at bit `off`; the words it fills completely are its
// own (plain stores), the first one if it starts inside it and the last one if it ends inside it are shared with its neighbours
// (atomicOr into the word k_jenc_scan cleared).
struct JeSink {
    uint32_t *w;
    unsigned long long acc;
    int n;
    bool shared;
    __device__ __forceinline__ void put(uint32_t code, int len)
    {
        acc = acc << len | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            const uint32_t v = (uint32_t)(acc >> n);
            if (shared)
                atomicOr(w, v);
            else
                *w = v;
            shared = false;
            w++;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (n > 0) atomicOr(w, (uint32_t)(acc << (32 - n)));
    }
};

// jchuff.c encode_one_block on the block's 64 coefficients (natural order, two per word).  EMIT: the bits go to the sink; else
// only their number is returned.
template <bool EMIT>
__device__ __forceinline__ uint32_t je_code_block(const uint32_t (&cw)[32], int diff, const uint32_t *dc, const uint32_t *ac, JeSink &sink)
{
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    uint32_t total = 0;
    {
        const int nb = 32 - __clz(abs(diff));  // (__clz(0) == 32)
        const uint32_t e = dc[nb];
        const uint32_t val = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u);
        total += (e >> 16) + nb;
        if (EMIT) sink.put((e & 0xffff) << nb | val, (int)(e >> 16) + nb);
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; k++) {
        const int v = (int)(int16_t)(cw[zz[k] >> 1] >> ((zz[k] & 1) * 16));
        if (v == 0) {
            run++;
            continue;
        }
        while (run > 15) {  // ZRL
            const uint32_t e = ac[0xF0];
            total += e >> 16;
            if (EMIT) sink.put(e & 0xffff, (int)(e >> 16));
            run -= 16;
        }
        const int nb = 32 - __clz(abs(v));
        const uint32_t e = ac[run << 4 | nb];
        const uint32_t val = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u);
        total += (e >> 16) + nb;
        if (EMIT) sink.put((e & 0xffff) << nb | val, (int)(e >> 16) + nb);
        run = 0;
    }
    if (run > 0) {  // EOB
        const uint32_t e = ac[0];
        total += e >> 16;
        if (EMIT) sink.put(e & 0xffff, (int)(e >> 16));
    }
    return total;
}

// EMIT false: lens[frame][s] = bits of block s, and the dummy blocks' DC written into coef.  EMIT true: the bits, at offs[frame][s].
template <bool EMIT>
__global__ __launch_bounds__(JE_TPB) void k_jenc_code(int16_t *__restrict__ coef, long long coef_fstride, uint32_t *__restrict__ lens,
                                                       const unsigned long long *__restrict__ offs, long long blk_fstride,
                                                       const JeFrame *__restrict__ info, uint32_t *__restrict__ bits, long long bits_fstride,
                                                       const JeTables *__restrict__ tab, const JeGeom G)
{
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    const int tid = threadIdx.x, f = blockIdx.y;
    for (int i = tid; i < 32; i += JE_TPB) (&s_dc[0][0])[i] = (&tab->dc[0][0])[i];
    for (int i = tid; i < 512; i += JE_TPB) (&s_ac[0][0])[i] = (&tab->ac[0][0])[i];
    __syncthreads();
    const int s = blockIdx.x * JE_TPB + tid;
    if (s >= G.nblk) return;
    if (EMIT && info[f].flags) return;  // (the frame does not fit: nothing of it is written)
    int16_t *fc = coef + (long long)f * coef_fstride;
    const JeBlockAt a = je_block_at(G, s);
    uint32_t cw[32];
    const uint4 *p = (const uint4 *)(fc + a.self * 64);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 v = p[j];
        cw[4 * j] = v.x;
        cw[4 * j + 1] = v.y;
        cw[4 * j + 2] = v.z;
        cw[4 * j + 3] = v.w;
    }
    int dcv = (int)(int16_t)(cw[0] & 0xffff);
    if (a.from >= 0) {  // a dummy block (all zero from k_jenc_dct): its DC is that of the block in front of it in the MCU
        dcv = fc[a.from * 64];
        if (!EMIT) fc[a.self * 64] = (int16_t)dcv;
    }
    const int pred = a.prev >= 0 ? (int)fc[a.prev * 64] : 0;
    const int t = a.c == 0 ? 0 : 1;
    JeSink sink;
    sink.w = nullptr;
    sink.acc = 0;
    sink.n = 0;
    sink.shared = false;
    if (EMIT) {
        const unsigned long long off = offs[(long long)f * blk_fstride + s];
        sink.w = bits + (long long)f * bits_fstride + (long long)(off >> 5);
        sink.n = (int)(off & 31);
        sink.shared = sink.n != 0;
    }
    const uint32_t total = je_code_block<EMIT>(cw, dcv - pred, s_dc[t], s_ac[t], sink);
    if (EMIT)
        sink.finish();
    else
        lens[(long long)f * blk_fstride + s] = total;
}

// ---------------------------------------------------------------- 3: bit offsets; 6: tile offsets of the stuffed bytes

__device__ __forceinline__ unsigned long long je_shfl_up64(unsigned long long v, int d)
{
    const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
    return (unsigned long long)hi << 32 | lo;
}

// exclusive scan of n 32-bit items into 64-bit sums by one workgroup of JE_SCAN_TPB lanes, JE_SCAN_TPB * JE_SCAN_PER items a round
// (the arrangement of k_jpeg_scan_blocks); returns the total in every lane.  out may alias nothing.
template <typename OUT>
__device__ __forceinline__ unsigned long long je_scan_items(const uint32_t *__restrict__ in, OUT *__restrict__ out, int n, unsigned long long *s_w)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += JE_SCAN_TPB * JE_SCAN_PER) {
        const int i0 = base + tid * JE_SCAN_PER;
        uint32_t item[JE_SCAN_PER];
        unsigned long long acc = 0;
#pragma unroll
        for (int k = 0; k < JE_SCAN_PER; k++) {
            item[k] = i0 + k < n ? in[i0 + k] : 0u;
            acc += item[k];
        }
        unsigned long long incl = acc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = je_shfl_up64(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        unsigned long long wpre = 0, tot = 0;
        for (int k = 0; k < JE_SCAN_TPB / 64; k++) {
            if (k == wv) wpre = tot;
            tot += s_w[k];
        }
        unsigned long long run = carry + wpre + incl - acc;
#pragma unroll
        for (int k = 0; k < JE_SCAN_PER; k++) {
            if (i0 + k < n) out[i0 + k] = (OUT)run;
            run += item[k];
        }
        carry += tot;
        __syncthreads();
    }
    return carry;
}

// bits_cap_bytes: entropy-coded bytes a frame's bit buffer holds (its words: that / 4 + 2, k_jenc_pack reads whole 16-byte groups)
__global__ __launch_bounds__(JE_SCAN_TPB) void k_jenc_scan(const uint32_t *__restrict__ lens, unsigned long long *__restrict__ offs, long long blk_fstride,
                                                            JeFrame *__restrict__ info, uint32_t *__restrict__ bits, long long bits_fstride,
                                                            unsigned long long bits_cap_bytes, int nblk)
{
    __shared__ unsigned long long s_w[JE_SCAN_TPB / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    const unsigned long long total = je_scan_items(lens + (long long)f * blk_fstride, offs + (long long)f * blk_fstride, nblk, s_w);
    const unsigned long long nbytes = (total + 7) >> 3;
    const bool over = nbytes > bits_cap_bytes;
    if (tid == 0) {
        info[f].bits = total;
        info[f].nbytes = 0;
        info[f].nff = 0;
        info[f].flags = over ? JE_OVER_BITS : 0u;
    }
    if (over) return;
    // every word the scan touches starts from zero, but for the 1-bits that fill the last byte (jchuff.c flush_bits)
    uint32_t *w = bits + (long long)f * bits_fstride;
    const unsigned long long nwords = (nbytes >> 2) + 2, last = total >> 5;
    const int fill = (int)((8 - (total & 7)) & 7);
    const uint32_t pad = fill ? ((1u << fill) - 1u) << (32 - (int)(total & 31) - fill) : 0u;
    for (unsigned long long i = tid; i < nwords; i += JE_SCAN_TPB) w[i] = i == last ? pad : 0u;
}

__device__ __forceinline__ uint32_t je_count_ff(const uint4 v, int nvalid)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) n += (k < nvalid && ((w[k >> 2] >> (24 - 8 * (k & 3))) & 255u) == 255u) ? 1u : 0u;
    return n;
}

__global__ __launch_bounds__(JE_TPB) void k_jenc_ffcount(const JeFrame *__restrict__ info, const uint32_t *__restrict__ bits, long long bits_fstride,
                                                          uint32_t *__restrict__ ffcnt, long long ff_fstride)
{
    __shared__ uint32_t s_n[JE_TPB / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (info[f].flags) return;
    const long long nbytes = (long long)((info[f].bits + 7) >> 3);
    const long long ntiles = (nbytes + JE_STUFF_TILE - 1) / JE_STUFF_TILE;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long i0 = tile * JE_STUFF_TILE + tid * 16;
        uint32_t n = 0;
        if (i0 < nbytes) n = je_count_ff(*(const uint4 *)(bits + (long long)f * bits_fstride + (i0 >> 2)), (int)min(16LL, nbytes - i0));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
        if ((tid & 63) == 0) s_n[tid >> 6] = n;
        __syncthreads();
        if (tid == 0) ffcnt[(long long)f * ff_fstride + tile] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(JE_SCAN_TPB) void k_jenc_ffscan(JeFrame *__restrict__ info, const uint32_t *__restrict__ ffcnt, uint32_t *__restrict__ ffoff,
                                                              long long ff_fstride, unsigned long long file_cap, int hdr_len)
{
    __shared__ unsigned long long s_w[JE_SCAN_TPB / 64];
    const int f = blockIdx.x;
    if (info[f].flags) return;
    const unsigned long long nbytes = (info[f].bits + 7) >> 3;
    const int ntiles = (int)((nbytes + JE_STUFF_TILE - 1) / JE_STUFF_TILE);
    const unsigned long long nff = je_scan_items(ffcnt + (long long)f * ff_fstride, ffoff + (long long)f * ff_fstride, ntiles, s_w);
    if (threadIdx.x == 0) {
        const unsigned long long file = (unsigned long long)hdr_len + nbytes + nff + 2;
        info[f].nff = (uint32_t)nff;
        info[f].nbytes = file;
        if (file > file_cap) info[f].flags = JE_OVER_FILE;
    }
}

// ---------------------------------------------------------------- 7: the file

__global__ __launch_bounds__(JE_TPB) void k_jenc_pack(const JeFrame *__restrict__ info, const uint32_t *__restrict__ bits, long long bits_fstride,
                                                       const uint32_t *__restrict__ ffoff, long long ff_fstride, const JeTables *__restrict__ tab, int hdr_len,
                                                       uint8_t *__restrict__ files, long long file_fstride)
{
    __shared__ uint32_t s_n[JE_TPB / 64];
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (info[f].flags) return;
    uint8_t *file = files + (long long)f * file_fstride;
    if (blockIdx.x == 0)
        for (int i = tid; i < hdr_len; i += JE_TPB) file[i] = tab->hdr[i];
    const long long nbytes = (long long)((info[f].bits + 7) >> 3);
    const long long ntiles = (nbytes + JE_STUFF_TILE - 1) / JE_STUFF_TILE;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long i0 = tile * JE_STUFF_TILE + tid * 16;
        const int nvalid = i0 < nbytes ? (int)min(16LL, nbytes - i0) : 0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (nvalid) v = *(const uint4 *)(bits + (long long)f * bits_fstride + (i0 >> 2));
        const uint32_t mine = je_count_ff(v, nvalid);
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_n[wv] = incl;
        __syncthreads();
        uint32_t before = ffoff[(long long)f * ff_fstride + tile] + incl - mine;
        for (int k = 0; k < wv; k++) before += s_n[k];
        uint8_t *dst = file + hdr_len + i0 + before;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < nvalid) {
                const uint8_t byte = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
                *dst++ = byte;
                if (byte == 255) *dst++ = 0;  // (jchuff.c emit_byte: a zero byte behind every 0xFF of the scan)
            }
        }
        if (nvalid && i0 + nvalid == nbytes) {  // EOI behind the last byte
            dst[0] = 0xFF;
            dst[1] = 0xD9;
        }
        __syncthreads();
    }
}

}  // namespace

// ---------------------------------------------------------------- the context

struct fid_jpeg_enc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int maxW = 0, maxH = 0, maxB = 0;
    int quality = 80, subsampling = 2;
    size_t file_cap = 0;      // max_file_bytes
    size_t file_stride = 0;   // bytes between the files on the device
    size_t bits_words = 0;    // words of a frame's bit buffer
    size_t max_blocks = 0, max_tiles = 0;
    int16_t *d_coef = nullptr;
    uint32_t *d_lens = nullptr, *d_bits = nullptr, *d_ffcnt = nullptr, *d_ffoff = nullptr;
    unsigned long long *d_offs = nullptr;
    uint8_t *d_files = nullptr, *d_src = nullptr;  // d_src: the frames of fid_jpeg_encode, made on its first call
    JeFrame *d_info = nullptr, *h_info = nullptr;
    JeTables *d_tab = nullptr, *h_tab = nullptr;
    long long tab_key = -1;  // what d_tab was made for
    JeGeom last;             // the last call, for the tap
    int last_n = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the seven launches of a call (fid_jpeg_enc_last_ms)
    float last_ms = 0.f;
    std::string last_error;
};

namespace {

struct JeBuffers {  // where the entropy stages of a launch group work: the context's arrays, or a larger bit buffer for one frame
    uint32_t *bits;
    long long bits_fstride;
    unsigned long long bits_cap_bytes;
    uint32_t *ffcnt, *ffoff;
    long long ff_fstride;
    long long max_tiles;
};

// launches 3 .. 7 for frames [f0, f0 + F) of the call (1 and 2 have run)
void je_launch_entropy(fid_jpeg_enc_ctx *c, const JeGeom &G, int f0, int F, const JeBuffers &B, bool pack)
{
    hipStream_t st = c->stream;
    const long long cs = (long long)c->max_blocks * 64, bs = (long long)c->max_blocks;
    int16_t *coef = c->d_coef + (long long)f0 * cs;
    uint32_t *lens = c->d_lens + (long long)f0 * bs;
    unsigned long long *offs = c->d_offs + (long long)f0 * bs;
    JeFrame *info = c->d_info + f0;
    hipLaunchKernelGGL(k_jenc_scan, dim3((unsigned)F), dim3(JE_SCAN_TPB), 0, st, lens, offs, bs, info, B.bits, B.bits_fstride, B.bits_cap_bytes, G.nblk);
    const dim3 gb((unsigned)((G.nblk + JE_TPB - 1) / JE_TPB), (unsigned)F);
    hipLaunchKernelGGL(k_jenc_code<true>, gb, dim3(JE_TPB), 0, st, coef, cs, lens, offs, bs, info, B.bits, B.bits_fstride, c->d_tab, G);
    long long gx = 2048 / F;
    gx = gx < 8 ? 8 : gx;
    gx = gx > B.max_tiles ? B.max_tiles : gx;
    const dim3 gt((unsigned)gx, (unsigned)F);
    hipLaunchKernelGGL(k_jenc_ffcount, gt, dim3(JE_TPB), 0, st, info, B.bits, B.bits_fstride, B.ffcnt, B.ff_fstride);
    hipLaunchKernelGGL(k_jenc_ffscan, dim3((unsigned)F), dim3(JE_SCAN_TPB), 0, st, info, B.ffcnt, B.ffoff, B.ff_fstride, (unsigned long long)c->file_cap, G.hdr_len);
    if (pack)
        hipLaunchKernelGGL(k_jenc_pack, gt, dim3(JE_TPB), 0, st, info, B.bits, B.bits_fstride, B.ffoff, B.ff_fstride, c->d_tab, G.hdr_len,
                           c->d_files + (size_t)f0 * c->file_stride, (long long)c->file_stride);
}

fid_status je_upload_tables(fid_jpeg_enc_ctx *c, const JeGeom &G)
{
    const long long key = ((((long long)c->quality * 4 + c->subsampling) * 4 + G.ncomp) << 32) | ((long long)G.W << 16) | G.H;
    if (key == c->tab_key) return FID_OK;
    JeTables *T = c->h_tab;
    for (int t = 0; t < 2; t++) {
        je_derive(kJeDcBits[t], kJeDcVals, T->dc[t], 16);
        je_derive(kJeAcBits[t], kJeAcVals[t], T->ac[t], 256);
        je_quant_table(t ? kJeStdChroma : kJeStdLuma, c->quality, T->q8[t]);
        for (int i = 0; i < 64; i++) {
            T->q8[t][i] *= 8;
            T->qm[t][i] = (uint32_t)(0x100000000ULL / T->q8[t][i]) + 1u;
        }
    }
    memset(T->hdr, 0, sizeof(T->hdr));
    je_header(c->quality, c->subsampling, G.W, G.H, G.ncomp, T->hdr);
    JPCHK(c, hipMemcpyAsync(c->d_tab, T, sizeof(JeTables), hipMemcpyHostToDevice, c->stream));
    JPCHK(c, hipStreamSynchronize(c->stream));  // (the pinned copy is rewritten by the next change of settings)
    c->tab_key = key;
    return FID_OK;
}

// the frames lie on the context's device at d_src; everything checked
fid_status je_encode(fid_jpeg_enc_ctx *c, const uint8_t *d_src, int F, int W, int H, int stride, long long fstride, fid_encoding enc, uint8_t *host_out,
                     int64_t host_file_stride, int64_t *nbytes_out)
{
    JeGeom G;
    je_geometry(W, H, enc == FID_ENC_MONO8 ? 1 : 3, c->subsampling, &G);
    G.enc = (int)enc;
    G.stride = stride;
    G.fstride = F > 1 ? fstride : 0;
    uint8_t hdr[JE_HDR_MAX];
    G.hdr_len = je_header(c->quality, c->subsampling, W, H, G.ncomp, hdr);
    c->last_n = 0;
    const fid_status rt = je_upload_tables(c, G);
    if (rt != FID_OK) return rt;
    hipStream_t st = c->stream;
    const long long cs = (long long)c->max_blocks * 64, bs = (long long)c->max_blocks;
    JPCHK(c, hipEventRecord(c->ev0, st));
    hipLaunchKernelGGL(k_jenc_dct, dim3((unsigned)((G.nblk + JE_DCT_BLOCKS - 1) / JE_DCT_BLOCKS), (unsigned)F), dim3(JE_TPB), 0, st, d_src, c->d_coef, cs,
                       c->d_tab, G);
    hipLaunchKernelGGL(k_jenc_code<false>, dim3((unsigned)((G.nblk + JE_TPB - 1) / JE_TPB), (unsigned)F), dim3(JE_TPB), 0, st, c->d_coef, cs, c->d_lens,
                       c->d_offs, bs, c->d_info, c->d_bits, (long long)c->bits_words, c->d_tab, G);
    const JeBuffers B = {c->d_bits, (long long)c->bits_words, (unsigned long long)c->file_cap, c->d_ffcnt, c->d_ffoff, (long long)c->max_tiles, (long long)c->max_tiles};
    je_launch_entropy(c, G, 0, F, B, true);
    JPCHK(c, hipGetLastError());
    JPCHK(c, hipEventRecord(c->ev1, st));
    JPCHK(c, hipMemcpyAsync(c->h_info, c->d_info, (size_t)F * sizeof(JeFrame), hipMemcpyDeviceToHost, st));
    JPCHK(c, hipStreamSynchronize(st));
    if (hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1) != hipSuccess) c->last_ms = 0.f;
    c->last = G;
    c->last_n = F;
    for (int f = 0; f < F; f++) {
        JeFrame I = c->h_info[f];
        if (I.flags & JE_OVER_BITS) {
            // the entropy-coded bytes alone are more than a file may have: code this frame once more into a buffer of the size it
            // needs, only to count its 0xFF bytes -- the refusal names the real size
            const unsigned long long nb = (I.bits + 7) >> 3;
            JeBuffers T;
            T.bits_fstride = (long long)(nb / 4 + 8);
            T.bits_cap_bytes = nb;
            T.max_tiles = (long long)(nb / JE_STUFF_TILE + 1);
            T.ff_fstride = T.max_tiles;
            T.bits = nullptr;
            T.ffcnt = nullptr;
            JPCHK(c, hipMalloc((void **)&T.bits, (size_t)T.bits_fstride * 4));
            const hipError_t e2 = hipMalloc((void **)&T.ffcnt, (size_t)T.max_tiles * 8);
            if (e2 != hipSuccess) {
                (void)hipFree(T.bits);
                JPCHK(c, e2);
            }
            T.ffoff = T.ffcnt + T.max_tiles;
            je_launch_entropy(c, G, f, 1, T, false);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(&c->h_info[f], c->d_info + f, sizeof(JeFrame), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            (void)hipFree(T.bits);
            (void)hipFree(T.ffcnt);
            JPCHK(c, e);
            I = c->h_info[f];
        }
        nbytes_out[f] = (int64_t)I.nbytes;
        if (I.flags || (int64_t)I.nbytes > host_file_stride) {
            char msg[200];
            snprintf(msg, sizeof msg, "frame %d needs %llu bytes: more than %s (%lld)", f, (unsigned long long)I.nbytes,
                     I.flags ? "the context's max_file_bytes" : "the caller's room per file", I.flags ? (long long)c->file_cap : (long long)host_file_stride);
            c->last_error = msg;
            return FID_E_CAPACITY;  // (nothing was copied: a file is whole or absent)
        }
    }
    for (int f = 0; f < F; f++)  // the copy is as long as the file, not as its room
        JPCHK(c, hipMemcpyAsync(host_out + (size_t)f * (size_t)host_file_stride, c->d_files + (size_t)f * c->file_stride, (size_t)c->h_info[f].nbytes,
                                hipMemcpyDeviceToHost, st));
    JPCHK(c, hipStreamSynchronize(st));
    return FID_OK;
}

fid_status je_check_call(fid_jpeg_enc_ctx *c, const void *frames, int F, int W, int H, int stride, long long fstride, fid_encoding enc, const void *host_out,
                         int64_t host_file_stride, const int64_t *nbytes_out, int *bpp)
{
    if (!c) return FID_E_INVALID_ARG;
    c->last_error.clear();
    if (enc != FID_ENC_MONO8 && enc != FID_ENC_BGR8 && enc != FID_ENC_RGB8) {
        c->last_error = "the encoder takes mono8, bgr8 and rgb8 frames";
        return FID_E_UNSUPPORTED;
    }
    *bpp = enc == FID_ENC_MONO8 ? 1 : 3;
    if (!frames || !host_out || !nbytes_out || F < 1 || F > c->maxB || W < 1 || H < 1 || W > c->maxW || H > c->maxH || host_file_stride < 1) {
        c->last_error = "null pointer, no frames, or more or larger frames than the context was created for";
        return FID_E_INVALID_ARG;
    }
    if ((long long)stride < (long long)W * *bpp || (F > 1 && fstride < 0)) {
        c->last_error = "stride_bytes is less than a row, or frame_stride_bytes is negative";
        return FID_E_INVALID_ARG;
    }
    return FID_OK;
}

}  // namespace

extern "C" {

fid_status fid_jpeg_enc_header(int32_t quality, int32_t subsampling, int32_t width, int32_t height, int32_t components, uint8_t *out, int64_t cap,
                               int64_t *nbytes)
{
    if (!nbytes || quality < 1 || quality > 100 || subsampling < 0 || subsampling > 2 || width < 1 || height < 1 || width > 65535 || height > 65535 ||
        (components != 1 && components != 3))
        return FID_E_INVALID_ARG;
    uint8_t hdr[JE_HDR_MAX];
    *nbytes = je_header(quality, subsampling, width, height, components, hdr);
    if (!out || cap < *nbytes) return FID_E_CAPACITY;
    memcpy(out, hdr, (size_t)*nbytes);
    return FID_OK;
}

void fid_jpeg_enc_destroy(fid_jpeg_enc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void *dev[] = {c->d_coef, c->d_lens, c->d_bits, c->d_ffcnt, c->d_ffoff, c->d_offs, c->d_files, c->d_src, c->d_info, c->d_tab};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (c->h_info) (void)hipHostFree(c->h_info);
    if (c->h_tab) (void)hipHostFree(c->h_tab);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

fid_status fid_jpeg_enc_create(int32_t device, int32_t max_width, int32_t max_height, int32_t max_batch, int64_t max_file_bytes, fid_jpeg_enc_ctx **out)
{
    if (!out || max_width < 1 || max_height < 1 || max_batch < 1 || max_width > 16384 || max_height > 16384 || max_file_bytes < 0) return FID_E_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FID_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return FID_E_INVALID_ARG;
    fid_jpeg_enc_ctx *c = new (std::nothrow) fid_jpeg_enc_ctx();
    if (!c) return FID_E_OUT_OF_MEMORY;
    c->device = device;
    c->maxW = max_width;
    c->maxH = max_height;
    c->maxB = max_batch;
    const size_t F = (size_t)max_batch;
    const size_t mw = ((size_t)max_width + 15) / 16 * 16, mh = ((size_t)max_height + 15) / 16 * 16;
    // max_file_bytes 0: the entropy-coded bytes a decoder context of the same size takes (fid_jpeg_create) and a header -- two bytes
    // a pixel of the MCU-padded frame, a third of the worst case above, some ten times a camera frame at quality 80 - 95
    c->file_cap = max_file_bytes > 0 ? (size_t)max_file_bytes : mw * mh * 2 + 65536 + JE_HDR_MAX;
    c->file_stride = (c->file_cap + 15) / 16 * 16;
    c->bits_words = (c->file_cap / 4 + 2 + 3) / 4 * 4 + 4;  // (whole 16-byte groups)
    c->max_blocks = mw * mh / 64 * 3;                       // 4:4:4 is the largest
    c->max_tiles = c->file_cap / JE_STUFF_TILE + 1;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess;
    ok = ok && hipMalloc((void **)&c->d_coef, F * c->max_blocks * 64 * sizeof(int16_t)) == hipSuccess &&
         hipMalloc((void **)&c->d_lens, F * c->max_blocks * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&c->d_offs, F * c->max_blocks * sizeof(unsigned long long)) == hipSuccess &&
         hipMalloc((void **)&c->d_bits, F * c->bits_words * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&c->d_ffcnt, F * c->max_tiles * sizeof(uint32_t)) == hipSuccess &&
         hipMalloc((void **)&c->d_ffoff, F * c->max_tiles * sizeof(uint32_t)) == hipSuccess && hipMalloc((void **)&c->d_files, F * c->file_stride) == hipSuccess &&
         hipMalloc((void **)&c->d_info, F * sizeof(JeFrame)) == hipSuccess && hipMalloc((void **)&c->d_tab, sizeof(JeTables)) == hipSuccess &&
         hipHostMalloc((void **)&c->h_info, F * sizeof(JeFrame)) == hipSuccess && hipHostMalloc((void **)&c->h_tab, sizeof(JeTables)) == hipSuccess;
    if (!ok) {
        fid_jpeg_enc_destroy(c);
        return FID_E_OUT_OF_MEMORY;
    }
    *out = c;
    return FID_OK;
}

const char *fid_jpeg_enc_last_error(fid_jpeg_enc_ctx *c) { return c ? c->last_error.c_str() : "null context"; }
float fid_jpeg_enc_last_ms(fid_jpeg_enc_ctx *c) { return c ? c->last_ms : 0.f; }

fid_status fid_jpeg_enc_set(fid_jpeg_enc_ctx *c, int32_t quality, int32_t subsampling)
{
    if (!c) return FID_E_INVALID_ARG;
    if (quality < 1 || quality > 100 || subsampling < 0 || subsampling > 2) {
        c->last_error = "quality is 1 .. 100, subsampling 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)";
        return FID_E_INVALID_ARG;
    }
    c->quality = quality;
    c->subsampling = subsampling;
    return FID_OK;
}

fid_status fid_jpeg_encode_device(fid_jpeg_enc_ctx *c, const void *d_frames, int32_t nframes, int32_t width, int32_t height, int32_t stride,
                                  int64_t frame_stride, fid_encoding enc, uint8_t *host_out, int64_t host_file_stride, int64_t *nbytes_out)
{
    int bpp = 0;
    const fid_status rc = je_check_call(c, d_frames, nframes, width, height, stride, frame_stride, enc, host_out, host_file_stride, nbytes_out, &bpp);
    if (rc != FID_OK) return rc;
    const unsigned long long frame = (unsigned long long)(height - 1) * (unsigned long long)stride + (unsigned long long)width * (unsigned)bpp;
    const unsigned long long span = (unsigned long long)(nframes - 1) * (unsigned long long)(nframes > 1 ? frame_stride : 0) + frame;
    if (draw_device_of((const uint8_t *)d_frames, span) != c->device) {
        c->last_error = "the frames are not memory of the context's device, or reach past their allocation";
        return FID_E_INVALID_ARG;
    }
    DrawDeviceScope scope(c->device);
    if (scope.rc != hipSuccess) return FID_E_HIP;
    return je_encode(c, (const uint8_t *)d_frames, nframes, width, height, stride, frame_stride, enc, host_out, host_file_stride, nbytes_out);
}

fid_status fid_jpeg_encode(fid_jpeg_enc_ctx *c, const uint8_t *frames, int32_t nframes, int32_t width, int32_t height, int32_t stride, int64_t frame_stride,
                           fid_encoding enc, uint8_t *host_out, int64_t host_file_stride, int64_t *nbytes_out)
{
    int bpp = 0;
    const fid_status rc = je_check_call(c, frames, nframes, width, height, stride, frame_stride, enc, host_out, host_file_stride, nbytes_out, &bpp);
    if (rc != FID_OK) return rc;
    DrawDeviceScope scope(c->device);
    if (scope.rc != hipSuccess) return FID_E_HIP;
    const size_t row = (size_t)width * (size_t)bpp, fbytes = row * (size_t)height;
    if (!c->d_src) JPCHK(c, hipMalloc((void **)&c->d_src, (size_t)c->maxB * (size_t)c->maxW * (size_t)c->maxH * 3));
    for (int f = 0; f < nframes; f++)  // tightly packed on the device
        JPCHK(c, hipMemcpy2DAsync(c->d_src + (size_t)f * fbytes, row, frames + (size_t)f * (size_t)(nframes > 1 ? frame_stride : 0), (size_t)stride, row,
                                  (size_t)height, hipMemcpyHostToDevice, c->stream));
    return je_encode(c, c->d_src, nframes, width, height, (int)row, (long long)fbytes, enc, host_out, host_file_stride, nbytes_out);
}

int64_t fid_jpeg_enc_tap_bytes(fid_jpeg_enc_ctx *c, int32_t frame)
{
    if (!c || frame < 0 || frame >= c->last_n) return 0;
    return (int64_t)c->last.nblk * 64 * (int64_t)sizeof(int16_t);
}

fid_status fid_jpeg_enc_tap_read(fid_jpeg_enc_ctx *c, int32_t frame, void *dst, int64_t dst_bytes)
{
    if (!c || !dst) return FID_E_INVALID_ARG;
    const int64_t nb = fid_jpeg_enc_tap_bytes(c, frame);
    if (nb == 0) {
        c->last_error = "fid_jpeg_enc_tap_read: no such frame in the last call";
        return FID_E_INVALID_ARG;
    }
    if (dst_bytes < nb) return FID_E_CAPACITY;
    DrawDeviceScope scope(c->device);
    if (scope.rc != hipSuccess) return FID_E_HIP;
    JPCHK(c, hipMemcpy(dst, c->d_coef + (size_t)frame * c->max_blocks * 64, (size_t)nb, hipMemcpyDeviceToHost));
    return FID_OK;
}

fid_status fid_jpeg_marker_jpeg(fid_jpeg_ctx *c, int32_t frame, fid_encoding base, const fid_marker *markers, int32_t n, uint32_t flags,
                                fid_jpeg_enc_ctx *e, uint8_t *out, int64_t cap, int64_t *nbytes)
{
    if (!c || !e || !out || !nbytes || cap < 1 || n < 0 || n > kDrawMaxMarkers || (n > 0 && !markers) || (flags & ~(uint32_t)FID_DRAW_FIRST_CORNER_LINE8))
        return FID_E_INVALID_ARG;
    if (base != FID_ENC_BGR8 && base != FID_ENC_MONO8) return FID_E_INVALID_ARG;
    if (c->last_n <= 0 || frame < 0 || frame >= c->last_n) {
        c->last_error = "fid_jpeg_marker_jpeg: no such frame in the last decode";
        return FID_E_INVALID_ARG;
    }
    if ((int)base != c->last_enc) {
        c->last_error = "fid_jpeg_marker_jpeg: the last decode made the other image (BGR8 / MONO8)";
        return FID_E_INVALID_ARG;
    }
    const int W = c->last_w, H = c->last_h, bpp = base == FID_ENC_MONO8 ? 1 : 3;
    if (e->device != c->device || W > e->maxW || H > e->maxH) {
        c->last_error = "fid_jpeg_marker_jpeg: the encoder context is on another device or smaller than the frame";
        return FID_E_INVALID_ARG;
    }
    // the marker image as fid_jpeg_marker_image makes it, in the decoder's buffer ...
    JPCHK(c, hipSetDevice(c->device));
    if (!c->d_mark) JPCHK(c, hipMalloc((void **)&c->d_mark, (size_t)c->maxW * c->maxH * 3));
    if (!c->d_mark_mk) JPCHK(c, hipMalloc((void **)&c->d_mark_mk, 16 + (size_t)kDrawMaxMarkers * 32));
    hipStream_t st = c->stream;
    fid_status rc = draw_launch_to_bgr(st, c->d_out + (size_t)frame * W * H * bpp, (long long)W * bpp, 0, base, c->d_mark, (long long)W * 3, 0, W, H, 1);
    std::vector<uint8_t> pack;
    if (rc == FID_OK && n > 0) {
        const size_t at = draw_pack(markers, n, &n, 1, &pack);
        JPCHK(c, hipMemcpyAsync(c->d_mark_mk, pack.data(), pack.size(), hipMemcpyHostToDevice, st));
        rc = draw_launch_markers(st, c->d_mark, W, H, (long long)W * 3, 0, c->d_mark_mk, at, 1, flags);
    }
    JPCHK(c, hipStreamSynchronize(st));
    if (rc != FID_OK) {
        c->last_error = "fid_jpeg_marker_jpeg: a kernel launch failed";
        return rc;
    }
    // ... and from there through the encoder: only the file crosses to the host
    e->last_error.clear();
    rc = je_encode(e, c->d_mark, 1, W, H, W * 3, 0, FID_ENC_BGR8, out, cap, nbytes);
    if (rc != FID_OK) c->last_error = "fid_jpeg_marker_jpeg: " + e->last_error;
    return rc;
}

}  // extern "C"
