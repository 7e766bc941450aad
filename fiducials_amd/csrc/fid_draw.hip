// fid_draw.hip -- the overlay of /fiducial_images: what imageCallback draws on its BGR8 copy of the
// frame before image_pub.publish (aruco_detect.cpp:381-387).  Part of the fid_api.hip translation unit.
//
// Host code first: the reference draws on the CPU too (aruco::drawDetectedMarkers on cv_ptr->image), the work is a few
// thousand pixels per frame, and for a raw frame the image is a host buffer on both sides of the call.  A frame that never
// reaches the host (a JPEG decoded on the device, a caller's frames in HBM) is drawn where it lies: k_to_bgr and k_draw_markers
// at the end of this file put the same bytes there (fid_to_bgr_device, fid_draw_detected_markers_device, fid_jpeg_marker_image).
//
// What is restated, exactly: cv::line(img, Point(p0), Point(p1), borderColor, thickness 1, LINE_8, shift 0) for the four sides
// of every marker -- drawing.cpp line() -> ThickLine() -> Line() -> LineIterator(img, pt1, pt2, 8, left_to_right = true), with
// clipLine() for end points outside the image; Point2f -> Point is saturate_cast<int> = cvRound (round half to even).
// What is NOT drawn (and is not claimed): the LINE_AA rectangle on the first corner and putText("id=<n>", FONT_HERSHEY_SIMPLEX,
// 0.5, thickness 2) -- LineAA's filter / slope-correction tables and the Hershey glyph tables are third-party data that is not
// in the reference tree nor on this machine, so they could not be pinned; aruco::drawAxis (:431, 3-px thick lines =
// FillConvexPoly + circles) likewise.  FID_DRAW_FIRST_CORNER_LINE8 adds the first-corner square as four LINE_8 lines in
// cornerColor for callers that want the cue -- those pixels are NOT the reference's (its square is anti-aliased).
#include <math.h>

#include <mutex>

namespace {

struct DrawPt {
    long long x, y;
};

// drawing.cpp clipLine(Size2l, Point2l&, Point2l&) -- for the host and the device alike: its truncating double divisions decide
// which pixels are drawn, so the device runs this very code
__host__ __device__ bool draw_clip_line(long long W, long long H, DrawPt &p1, DrawPt &p2)
{
    const long long right = W - 1, bottom = H - 1;
    if (W <= 0 || H <= 0) return false;
    long long &x1 = p1.x, &y1 = p1.y, &x2 = p2.x, &y2 = p2.y;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (x2 - x1) / (y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (x2 - x1) / (y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (y2 - y1) / (x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (y2 - y1) / (x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// Line(): LineIterator(img, pt1, pt2, connectivity 8, left_to_right true), three bytes per pixel
void draw_line8(uint8_t *img, int W, int H, long long stride, DrawPt a, DrawPt b, const uint8_t color[3])
{
    if ((unsigned long long)a.x >= (unsigned long long)W || (unsigned long long)b.x >= (unsigned long long)W ||
        (unsigned long long)a.y >= (unsigned long long)H || (unsigned long long)b.y >= (unsigned long long)H)
        if (!draw_clip_line(W, H, a, b)) return;
    // clipLine() does not look at y again after the x clip; with end points near +-2^31 its double arithmetic is off by hundreds
    // of pixels and the reference would write outside its image there.  Such a line is left out instead.
    if ((unsigned long long)a.x >= (unsigned long long)W || (unsigned long long)b.x >= (unsigned long long)W ||
        (unsigned long long)a.y >= (unsigned long long)H || (unsigned long long)b.y >= (unsigned long long)H)
        return;
    long long dx = b.x - a.x, dy = b.y - a.y;
    long long s = dx < 0 ? -1 : 0;
    // left_to_right: the walk starts at the end point with the smaller x
    dx = (dx ^ s) - s;
    dy = (dy ^ s) - s;
    a.x ^= (a.x ^ b.x) & s;
    a.y ^= (a.y ^ b.y) & s;
    uint8_t *ptr = img + a.y * stride + a.x * 3;
    long long bt_pix = 3, istep = stride;
    s = dy < 0 ? -1 : 0;
    dy = (dy ^ s) - s;
    istep = (istep ^ s) - s;
    s = dy > dx ? -1 : 0;
    // conditional swaps
    dx ^= dy & s;
    dy ^= dx & s;
    dx ^= dy & s;
    bt_pix ^= istep & s;
    istep ^= bt_pix & s;
    bt_pix ^= istep & s;
    long long err = dx - (dy + dy);
    const long long plusDelta = dx + dx, minusDelta = -(dy + dy), plusStep = istep, minusStep = bt_pix;
    const long long count = dx + 1;
    for (long long i = 0; i < count; i++) {
        ptr[0] = color[0];
        ptr[1] = color[1];
        ptr[2] = color[2];
        const long long mask = err < 0 ? -1 : 0;
        err += minusDelta + (plusDelta & mask);
        ptr += minusStep + (plusStep & mask);
    }
}

// Point2f -> Point: saturate_cast<int>(float) = cvRound = cvtss2si on the reference's x86-64 build: round to nearest even, and
// the "integer indefinite" INT_MIN for NaN, +-inf and everything outside the int range (CORNER_REFINE_CONTOUR crosses two
// fitted lines: near-parallel ones give such corners).  The result always fits 32 bits, so the 64-bit line arithmetic below
// (OpenCV's own Point2l) cannot overflow.
inline long long draw_cv_round(float v)
{
    if (!(v >= -2147483648.f && v < 2147483648.f)) return -2147483648LL;  // (NaN fails both comparisons)
    return (long long)lrintf(v);
}

}  // namespace

extern "C" {

fid_status fid_to_bgr(const uint8_t *img, int32_t width, int32_t height, int32_t stride, fid_encoding enc, uint8_t *out_bgr, int64_t out_bytes)
{
    if (!img || !out_bgr || width < 1 || height < 1) return FID_E_INVALID_ARG;
    const int bpp = enc == FID_ENC_MONO8 ? 1 : ((enc == FID_ENC_BGRA8 || enc == FID_ENC_RGBA8) ? 4 : 3);
    if (enc != FID_ENC_MONO8 && enc != FID_ENC_BGR8 && enc != FID_ENC_RGB8 && enc != FID_ENC_BGRA8 && enc != FID_ENC_RGBA8) return FID_E_INVALID_ARG;
    if ((int64_t)stride < (int64_t)width * bpp) return FID_E_INVALID_ARG;  // (64-bit: width * bpp wraps for absurd widths)
    if (out_bytes < (int64_t)width * height * 3) return FID_E_CAPACITY;
    const bool swap = enc == FID_ENC_RGB8 || enc == FID_ENC_RGBA8;
    for (int y = 0; y < height; y++) {
        const uint8_t *s = img + (size_t)y * stride;
        uint8_t *o = out_bgr + (size_t)y * width * 3;
        if (enc == FID_ENC_MONO8) {
            for (int x = 0; x < width; x++) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = s[x];  // cvtColor(GRAY2BGR)
        } else {
            for (int x = 0; x < width; x++) {
                const uint8_t *p = s + (size_t)x * bpp;
                o[3 * x] = swap ? p[2] : p[0];
                o[3 * x + 1] = p[1];
                o[3 * x + 2] = swap ? p[0] : p[2];
            }
        }
    }
    return FID_OK;
}

// ---- cv_bridge::toCvCopy(msg, "bgr8") for the encodings a raw (uncompressed) camera driver publishes beside the five the device
// path takes itself (aruco_detect.cpp:348).  cv_bridge.cpp toCvCopy -> convertColor: a list of conversions by (source, target)
// format -- cvtColor for the colour layout, then, when the bit depths differ, Mat::convertTo(8U, 255. / 65535.).
//   * mono16 / bgr16 / rgb16 / bgra16 / rgba16: layout first (GRAY2BGR / RGB2BGR / BGRA2BGR / RGBA2BGR are pure channel moves),
//     then every sample through convertTo: cvtScale<ushort, uchar, float> = saturate_cast<uchar>(cvRound(v * (float)(255. / 65535.)))
//     with the product formed in float; big-endian messages are byte-swapped first (cv_bridge does so when the host differs);
//   * bayer_rggb8 / bayer_bggr8 / bayer_gbrg8 / bayer_grbg8: cv_bridge maps them to COLOR_BayerBG / RG / GR / GB2BGR (OpenCV names a
//     pattern by the pixels at (1,1),(1,2)); cv::demosaicing's bilinear Bayer2RGB_<uchar>: an interior pixel keeps its own colour,
//     the other two are (a + b + 1) >> 1 of the two or (a + b + c + d + 2) >> 2 of the four nearest samples of that colour; the
//     first / last column of an interior row repeat their neighbour, then the first / last row repeat theirs; an image of
//     height <= 2 comes out black.
// Restated from the published OpenCV 4.2 / cv_bridge (noetic) sources, which are not on this machine: PARITY UNPINNED (no
// reference fixture uses these encodings); tests/test_overlay.py checks them against an independent statement of the same rules.
//   * yuv422 (UYVY): cvtColor(COLOR_YUV2BGR_UYVY), BT.601 in 20-bit fixed point (below).
// The 16-bit Bayer encodings and everything else stay FID_E_UNSUPPORTED: the node reports them like the cv_bridge exception it
// would catch.
static inline uint8_t cvb_scale_16_to_8(uint16_t v)
{
    const float a = (float)(255. / 65535.);
    const float p = (float)v * a;
    const long r = lrintf(p);  // cvRound: nearest, ties to even
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

static void cvb_bayer_to_bgr(const uint8_t *src, int W, int H, long long step, int blue0, int green0, uint8_t *dst)
{
    const long long ds = (long long)W * 3;
    if (H <= 2 || W <= 2) {
        // (height <= 2: both border rows are written as zeros and nothing lies between them; width <= 2 is refused by the caller)
        memset(dst, 0, (size_t)ds * (size_t)H);
        return;
    }
    int blue = blue0, start_with_green = green0;
    for (int i = 0; i < H - 2; i++) {
        const uint8_t *bayer = src + (long long)i * step;
        const uint8_t *bayer_end = bayer + (W - 2);
        uint8_t *dst0 = dst + (long long)(i + 1) * ds + 3 + 1;  // pixel (i + 1, 1), its middle (green) channel
        uint8_t *d = dst0;
        const long long bs = step;
        int t0, t1;
        if (start_with_green) {
            t0 = (bayer[1] + bayer[bs * 2 + 1] + 1) >> 1;
            t1 = (bayer[bs] + bayer[bs + 2] + 1) >> 1;
            d[-blue] = (uint8_t)t0;
            d[0] = bayer[bs + 1];
            d[blue] = (uint8_t)t1;
            bayer++;
            d += 3;
        }
        for (; bayer <= bayer_end - 2; bayer += 2, d += 6) {
            t0 = (bayer[0] + bayer[2] + bayer[bs * 2] + bayer[bs * 2 + 2] + 2) >> 2;
            t1 = (bayer[1] + bayer[bs] + bayer[bs + 2] + bayer[bs * 2 + 1] + 2) >> 2;
            d[-blue] = (uint8_t)t0;
            d[0] = (uint8_t)t1;
            d[blue] = bayer[bs + 1];
            t0 = (bayer[2] + bayer[bs * 2 + 2] + 1) >> 1;
            t1 = (bayer[bs + 1] + bayer[bs + 3] + 1) >> 1;
            d[3 - blue] = (uint8_t)t0;  // (the green pixel beside it: its vertical pair is the colour this row does not carry,
            d[3] = bayer[bs + 2];       //  its horizontal pair the colour of the pixel before it)
            d[3 + blue] = (uint8_t)t1;
        }
        if (bayer < bayer_end) {
            t0 = (bayer[0] + bayer[2] + bayer[bs * 2] + bayer[bs * 2 + 2] + 2) >> 2;
            t1 = (bayer[1] + bayer[bs] + bayer[bs + 2] + bayer[bs * 2 + 1] + 2) >> 2;
            d[-blue] = (uint8_t)t0;
            d[0] = (uint8_t)t1;
            d[blue] = bayer[bs + 1];
        }
        // the first and the last pixel of the row repeat their neighbours
        dst0[-4] = dst0[-1];
        dst0[-3] = dst0[0];
        dst0[-2] = dst0[1];
        dst0[(W - 2) * 3 - 1] = dst0[(W - 2) * 3 - 4];
        dst0[(W - 2) * 3] = dst0[(W - 2) * 3 - 3];
        dst0[(W - 2) * 3 + 1] = dst0[(W - 2) * 3 - 2];
        blue = -blue;
        start_with_green = !start_with_green;
    }
    for (long long k = 0; k < ds; k++) {  // the first and the last row repeat theirs
        dst[k] = dst[k + ds];
        dst[k + (long long)(H - 1) * ds] = dst[k + (long long)(H - 2) * ds];
    }
}

fid_status fid_image_to_bgr8(const uint8_t *img, int32_t width, int32_t height, int32_t stride, const char *encoding, int32_t is_bigendian,
                             uint8_t *out_bgr, int64_t out_bytes)
{
    if (!img || !out_bgr || !encoding || width < 1 || height < 1 || width > 32767 || height > 32767) return FID_E_INVALID_ARG;
    if (out_bytes < (int64_t)width * height * 3) return FID_E_CAPACITY;
    const std::string e(encoding);
    static const struct { const char *name; fid_encoding enc; } eight[] = {
        {"mono8", FID_ENC_MONO8}, {"bgr8", FID_ENC_BGR8}, {"rgb8", FID_ENC_RGB8}, {"bgra8", FID_ENC_BGRA8}, {"rgba8", FID_ENC_RGBA8}};
    for (const auto &k : eight)
        if (e == k.name) return fid_to_bgr(img, width, height, stride, k.enc, out_bgr, out_bytes);
    int ch = 0, swap = 0;
    if (e == "mono16") ch = 1;
    else if (e == "bgr16") ch = 3;
    else if (e == "rgb16") ch = 3, swap = 1;
    else if (e == "bgra16") ch = 4;
    else if (e == "rgba16") ch = 4, swap = 1;
    if (ch) {
        if ((int64_t)stride < (int64_t)width * ch * 2) return FID_E_INVALID_ARG;
        const bool be = is_bigendian != 0;
        for (int y = 0; y < height; y++) {
            const uint8_t *s = img + (size_t)y * (size_t)stride;
            uint8_t *o = out_bgr + (size_t)y * (size_t)width * 3;
            for (int x = 0; x < width; x++) {
                uint8_t v[4] = {0, 0, 0, 0};
                for (int k = 0; k < ch; k++) {
                    const uint8_t *p = s + ((size_t)x * ch + k) * 2;
                    v[k] = cvb_scale_16_to_8(be ? (uint16_t)((p[0] << 8) | p[1]) : (uint16_t)(p[0] | (p[1] << 8)));
                }
                if (ch == 1) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = v[0];
                else {
                    o[3 * x] = swap ? v[2] : v[0];
                    o[3 * x + 1] = v[1];
                    o[3 * x + 2] = swap ? v[0] : v[2];
                }
            }
        }
        return FID_OK;
    }
    if (e == "yuv422") {
        // cv_bridge: YUV422 -> BGR8 is cvtColor(COLOR_YUV2BGR_UYVY): U0 Y0 V0 Y1 per pixel pair, ITU-R BT.601 in 20-bit fixed point
        // (imgproc color_yuv: ITUR_BT_601_CY 1220542, CUB 2116026, CUG -409993, CVG -852492, CVR 1673527; y = max(0, Y - 16) * CY;
        //  channel = saturate((y + (1 << 19) + coefficient sums of (U - 128), (V - 128)) >> 20)).  Width must be even.
        if ((width & 1) || (int64_t)stride < (int64_t)width * 2) return FID_E_INVALID_ARG;
        const int CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527, SH = 20;
        auto sat = [](int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
        for (int y = 0; y < height; y++) {
            const uint8_t *sp = img + (size_t)y * (size_t)stride;
            uint8_t *o = out_bgr + (size_t)y * (size_t)width * 3;
            for (int x = 0; x < width; x += 2) {
                const int u = sp[2 * x] - 128, y0 = sp[2 * x + 1], v = sp[2 * x + 2] - 128, y1 = sp[2 * x + 3];
                const int ruv = (1 << (SH - 1)) + CVR * v, guv = (1 << (SH - 1)) + CVG * v + CUG * u, buv = (1 << (SH - 1)) + CUB * u;
                const int a0 = (y0 - 16 > 0 ? y0 - 16 : 0) * CY, a1 = (y1 - 16 > 0 ? y1 - 16 : 0) * CY;
                o[3 * x] = sat((a0 + buv) >> SH);
                o[3 * x + 1] = sat((a0 + guv) >> SH);
                o[3 * x + 2] = sat((a0 + ruv) >> SH);
                o[3 * x + 3] = sat((a1 + buv) >> SH);
                o[3 * x + 4] = sat((a1 + guv) >> SH);
                o[3 * x + 5] = sat((a1 + ruv) >> SH);
            }
        }
        return FID_OK;
    }
    int blue = 0, green = 0;
    if (e == "bayer_rggb8") blue = -1, green = 0;       // COLOR_BayerBG2BGR
    else if (e == "bayer_bggr8") blue = 1, green = 0;   // COLOR_BayerRG2BGR
    else if (e == "bayer_gbrg8") blue = 1, green = 1;   // COLOR_BayerGR2BGR
    else if (e == "bayer_grbg8") blue = -1, green = 1;  // COLOR_BayerGB2BGR
    if (blue) {
        if (stride < width || width < 3) return FID_E_INVALID_ARG;
        cvb_bayer_to_bgr(img, width, height, stride, blue, green, out_bgr);
        return FID_OK;
    }
    return FID_E_UNSUPPORTED;
}

fid_status fid_encoding_from_string(const char *encoding, int32_t is_bigendian, fid_encoding *out_enc, int32_t *bytes_per_pixel)
{
    if (!encoding || !out_enc) return FID_E_INVALID_ARG;
    static const struct { const char *name; int enc, bpp; } tab[] = {
        {"mono8", FID_ENC_MONO8, 1}, {"bgr8", FID_ENC_BGR8, 3}, {"rgb8", FID_ENC_RGB8, 3}, {"bgra8", FID_ENC_BGRA8, 4}, {"rgba8", FID_ENC_RGBA8, 4},
        {"bayer_rggb8", FID_ENC_BAYER_RGGB8, 1}, {"bayer_bggr8", FID_ENC_BAYER_BGGR8, 1}, {"bayer_gbrg8", FID_ENC_BAYER_GBRG8, 1},
        {"bayer_grbg8", FID_ENC_BAYER_GRBG8, 1}, {"mono16", FID_ENC_MONO16, 2}, {"bgr16", FID_ENC_BGR16, 6}, {"rgb16", FID_ENC_RGB16, 6},
        {"bgra16", FID_ENC_BGRA16, 8}, {"rgba16", FID_ENC_RGBA16, 8}, {"yuv422", FID_ENC_YUV422, 2}};
    for (const auto &t : tab)
        if (!strcmp(encoding, t.name)) {
            const bool wide = t.enc >= FID_ENC_MONO16 && t.enc <= FID_ENC_RGBA16;
            *out_enc = (fid_encoding)(t.enc | (wide && is_bigendian ? FID_ENC_BIGENDIAN : 0));
            if (bytes_per_pixel) *bytes_per_pixel = t.bpp;
            return FID_OK;
        }
    return FID_E_UNSUPPORTED;
}

fid_status fid_draw_detected_markers(uint8_t *bgr, int32_t width, int32_t height, int32_t stride, const fid_marker *markers, int32_t n,
                                     uint32_t flags)
{
    if (!bgr || width < 1 || height < 1 || (int64_t)stride < (int64_t)width * 3 || n < 0 || (n > 0 && !markers)) return FID_E_INVALID_ARG;
    if (flags & ~(uint32_t)FID_DRAW_FIRST_CORNER_LINE8) return FID_E_INVALID_ARG;
    // borderColor = Scalar(0, 255, 0) (the default imageCallback leaves in place); cornerColor = borderColor with val[1] and
    // val[2] swapped (drawDetectedMarkers; its own comment says "G and B", the code swaps G and R): (0, 0, 255) = red in BGR
    const uint8_t border[3] = {0, 255, 0}, corner[3] = {0, 0, 255};
    for (int i = 0; i < n; i++) {
        const float *c = markers[i].corners;
        for (int j = 0; j < 4; j++) {
            const int k = (j + 1) & 3;
            const DrawPt p0 = {draw_cv_round(c[2 * j]), draw_cv_round(c[2 * j + 1])}, p1 = {draw_cv_round(c[2 * k]), draw_cv_round(c[2 * k + 1])};
            draw_line8(bgr, width, height, stride, p0, p1, border);
        }
        if (flags & FID_DRAW_FIRST_CORNER_LINE8) {
            // rectangle(img, c0 - (3, 3), c0 + (3, 3), cornerColor, 1, LINE_AA) drawn with LINE_8 sides instead: NOT the reference's pixels
            const float x0 = c[0] - 3.f, y0 = c[1] - 3.f, x1 = c[0] + 3.f, y1 = c[1] + 3.f;
            const DrawPt q[4] = {{draw_cv_round(x0), draw_cv_round(y0)}, {draw_cv_round(x1), draw_cv_round(y0)}, {draw_cv_round(x1), draw_cv_round(y1)},
                                 {draw_cv_round(x0), draw_cv_round(y1)}};
            for (int j = 0; j < 4; j++) draw_line8(bgr, width, height, stride, q[j], q[(j + 1) & 3], corner);
        }
    }
    return FID_OK;
}

}  // extern "C"

// =====================================================================================================================
// The overlay on the device: the same bytes as fid_to_bgr / fid_draw_detected_markers, for frames that lie in device memory.
// =====================================================================================================================
namespace {

// the most markers one frame can carry on any context (max_markers_per_frame <= max_candidates_per_frame <= 4096, fid_create)
constexpr int kDrawMaxMarkers = 4096;

int draw_enc_bpp(fid_encoding enc)
{
    switch (enc) {
    case FID_ENC_MONO8: return 1;
    case FID_ENC_BGR8: case FID_ENC_RGB8: return 3;
    case FID_ENC_BGRA8: case FID_ENC_RGBA8: return 4;
    default: return 0;  // (what fid_to_bgr refuses)
    }
}

// ---- k_to_bgr: toCvCopy(BGR8) of F frames with any source / destination row and frame strides.  A lane converts 16 pixels of a
// row: 16-byte loads and stores where both rows' addresses are 16-byte aligned and the 16 pixels are whole, single bytes otherwise
// (a row's tail, odd strides).  BPP and SWAP are template arguments so that every byte index is a constant (no scratch).
template <int BPP, bool SWAP>
__global__ __launch_bounds__(256) void k_to_bgr(const uint8_t *__restrict__ src, long long sstride, long long sfstride, uint8_t *__restrict__ dst,
                                                long long dstride, long long dfstride, int W, int H, int F)
{
    const long long cpr = (W + 15) >> 4;
    const long long chunks = cpr * H;
    for (int f = blockIdx.y; f < F; f += gridDim.y) {
        for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (long long)gridDim.x * blockDim.x) {
            const long long y = c / cpr;
            const int x0 = (int)(c - y * cpr) * 16;
            const uint8_t *s = src + f * sfstride + y * sstride + (long long)x0 * BPP;
            uint8_t *d = dst + f * dfstride + y * dstride + (long long)x0 * 3;
            if (x0 + 16 <= W && (((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
                uint4 in[BPP];
#pragma unroll
                for (int k = 0; k < BPP; k++) in[k] = ((const uint4 *)s)[k];
                const uint8_t *ib = (const uint8_t *)in;
                uint4 out[3];
                uint8_t *ob = (uint8_t *)out;
#pragma unroll
                for (int p = 0; p < 16; p++) {
                    const uint8_t *q = ib + p * BPP;
                    ob[3 * p] = BPP == 1 ? q[0] : (SWAP ? q[2] : q[0]);
                    ob[3 * p + 1] = BPP == 1 ? q[0] : q[1];
                    ob[3 * p + 2] = BPP == 1 ? q[0] : (SWAP ? q[0] : q[2]);
                }
#pragma unroll
                for (int k = 0; k < 3; k++) ((uint4 *)d)[k] = out[k];
            } else {
                const int x1 = x0 + 16 < W ? x0 + 16 : W;
                for (int x = x0; x < x1; x++, s += BPP, d += 3) {
                    const uint8_t b = BPP == 1 ? s[0] : (SWAP ? s[2] : s[0]), g = BPP == 1 ? s[0] : s[1], r = BPP == 1 ? s[0] : (SWAP ? s[0] : s[2]);
                    d[0] = b;
                    d[1] = g;
                    d[2] = r;
                }
            }
        }
    }
}

fid_status draw_launch_to_bgr(hipStream_t st, const uint8_t *s, long long sstride, long long sfstride, fid_encoding enc, uint8_t *d, long long dstride,
                              long long dfstride, int W, int H, int F)
{
    const long long chunks = (long long)((W + 15) / 16) * H;
    const long long bx = (chunks + 255) / 256;
    const dim3 grid((unsigned)(bx < 1024 ? bx : 1024), (unsigned)(F < 65535 ? F : 65535)), block(256);
    switch (enc) {
    case FID_ENC_MONO8: hipLaunchKernelGGL((k_to_bgr<1, false>), grid, block, 0, st, s, sstride, sfstride, d, dstride, dfstride, W, H, F); break;
    case FID_ENC_BGR8: hipLaunchKernelGGL((k_to_bgr<3, false>), grid, block, 0, st, s, sstride, sfstride, d, dstride, dfstride, W, H, F); break;
    case FID_ENC_RGB8: hipLaunchKernelGGL((k_to_bgr<3, true>), grid, block, 0, st, s, sstride, sfstride, d, dstride, dfstride, W, H, F); break;
    case FID_ENC_BGRA8: hipLaunchKernelGGL((k_to_bgr<4, false>), grid, block, 0, st, s, sstride, sfstride, d, dstride, dfstride, W, H, F); break;
    case FID_ENC_RGBA8: hipLaunchKernelGGL((k_to_bgr<4, true>), grid, block, 0, st, s, sstride, sfstride, d, dstride, dfstride, W, H, F); break;
    default: return FID_E_INVALID_ARG;
    }
    return hipGetLastError() == hipSuccess ? FID_OK : FID_E_HIP;
}

// ---- k_draw_markers: draw_line8 without its serial walk.  draw_seg applies the host's normalisation (clipLine, left to right, the
// sign of the minor axis folded into the step, the axes swapped so that 0 <= dmin <= dmaj); pixel i of dmaj + 1 is then at major
// offset i and minor offset floor((2 i dmin + dmaj - 1) / (2 dmaj)) -- where the err walk of draw_line8 puts it.  64-bit as there.
struct DrawSeg {
    long long x0, y0, dmaj, dmin, count;
    int sy, swap;
};

__device__ inline long long draw_cv_round_dev(float v)
{
    if (!(v >= -2147483648.f && v < 2147483648.f)) return -2147483648LL;  // (as draw_cv_round: NaN fails both comparisons)
    return (long long)rintf(v);                                            // (nearest, ties to even: lrintf)
}

__device__ inline bool draw_inside(long long W, long long H, const DrawPt &a, const DrawPt &b)
{
    return (unsigned long long)a.x < (unsigned long long)W && (unsigned long long)b.x < (unsigned long long)W &&
           (unsigned long long)a.y < (unsigned long long)H && (unsigned long long)b.y < (unsigned long long)H;
}

__device__ bool draw_seg(long long W, long long H, DrawPt a, DrawPt b, DrawSeg &g)
{
    if (!draw_inside(W, H, a, b) && !draw_clip_line(W, H, a, b)) return false;
    if (!draw_inside(W, H, a, b)) return false;  // (what draw_line8 leaves out after clipLine)
    long long dx = b.x - a.x, dy = b.y - a.y;
    if (dx < 0) {  // left_to_right
        a = b;
        dx = -dx;
        dy = -dy;
    }
    g.sy = dy < 0 ? -1 : 1;
    dy = dy < 0 ? -dy : dy;
    g.swap = dy > dx;
    g.dmaj = g.swap ? dy : dx;
    g.dmin = g.swap ? dx : dy;
    g.x0 = a.x;
    g.y0 = a.y;
    g.count = g.dmaj + 1;
    return true;
}

// the pixels of one line, spread over the 64 lanes of a wave (every end point is inside the image: so is every pixel)
__device__ void draw_seg_wave(uint8_t *fr, long long W, long long H, long long stride, DrawPt a, DrawPt b, uint8_t c0, uint8_t c1, uint8_t c2, int lane)
{
    DrawSeg g;
    if (!draw_seg(W, H, a, b, g)) return;
    const long long den = 2 * g.dmaj;
    for (long long i = lane; i < g.count; i += 64) {
        const long long m = den ? (2 * i * g.dmin + g.dmaj - 1) / den : 0;
        const long long x = g.x0 + (g.swap ? m : i), y = g.y0 + g.sy * (g.swap ? i : m);
        uint8_t *p = fr + y * stride + x * 3;
        p[0] = c0;
        p[1] = c1;
        p[2] = c2;
    }
}

// side j of a marker (corner j -> corner j + 1) in (0, 255, 0); with `square`, side j of the first-corner square in (0, 0, 255)
__device__ inline void draw_side(uint8_t *fr, long long W, long long H, long long stride, const float *c, int j, bool square, int lane)
{
    if (!square) {
        const int k = (j + 1) & 3;
        const DrawPt p0 = {draw_cv_round_dev(c[2 * j]), draw_cv_round_dev(c[2 * j + 1])}, p1 = {draw_cv_round_dev(c[2 * k]), draw_cv_round_dev(c[2 * k + 1])};
        draw_seg_wave(fr, W, H, stride, p0, p1, 0, 255, 0, lane);
    } else {
        const float x0 = c[0] - 3.f, y0 = c[1] - 3.f, x1 = c[0] + 3.f, y1 = c[1] + 3.f;
        const long long X0 = draw_cv_round_dev(x0), Y0 = draw_cv_round_dev(y0), X1 = draw_cv_round_dev(x1), Y1 = draw_cv_round_dev(y1);
        const DrawPt q0 = {j == 1 || j == 2 ? X1 : X0, j >= 2 ? Y1 : Y0};  // q[j] of {(x0,y0), (x1,y0), (x1,y1), (x0,y1)}
        const int k = (j + 1) & 3;
        const DrawPt q1 = {k == 1 || k == 2 ? X1 : X0, k >= 2 ? Y1 : Y0};
        draw_seg_wave(fr, W, H, stride, q0, q1, 0, 0, 255, lane);
    }
}

// One workgroup per frame (a grid-stride loop over frames), one wave per line.  Frame f's markers are corners[first[f] ..
// first[f + 1]), 8 floats each.  Without the square every write is the same colour and the lines go in any order.  With it, two
// colours can meet on a pixel and the host's order decides (marker i's sides, its square, marker i + 1's sides, ...): a barrier
// between the colours makes the last writer the host's.
__global__ __launch_bounds__(256) void k_draw_markers(uint8_t *__restrict__ img, int W, int H, long long stride, long long fstride,
                                                      const float *__restrict__ corners, const int *__restrict__ first, int F, int square)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        uint8_t *fr = img + (long long)f * fstride;
        const int m0 = first[f], n = first[f + 1] - m0;
        if (!square) {
            for (int l = wave; l < 4 * n; l += nw) draw_side(fr, W, H, stride, corners + (size_t)(m0 + (l >> 2)) * 8, l & 3, false, lane);
        } else {
            for (int i = 0; i < n; i++) {
                const float *c = corners + (size_t)(m0 + i) * 8;
                for (int j = wave; j < 4; j += nw) draw_side(fr, W, H, stride, c, j, false, lane);
                __syncthreads();
                for (int j = wave; j < 4; j += nw) draw_side(fr, W, H, stride, c, j, true, lane);
                __syncthreads();
            }
        }
    }
}

// the markers of F frames as k_draw_markers reads them: int32 first[F + 1], then (16-byte aligned) 8 floats per marker.
// Returns the offset of the corners.
size_t draw_pack(const fid_marker *markers, int32_t cap_per_frame, const int32_t *n_per_frame, int32_t F, std::vector<uint8_t> *buf)
{
    const size_t at = ((size_t)(F + 1) * 4 + 15) & ~(size_t)15;
    int64_t total = 0;
    for (int f = 0; f < F; f++) total += n_per_frame[f];
    buf->assign(at + (size_t)total * 32, 0);
    int32_t *first = (int32_t *)buf->data();
    float *c = (float *)(buf->data() + at);
    int32_t k = 0;
    for (int f = 0; f < F; f++) {
        first[f] = k;
        for (int i = 0; i < n_per_frame[f]; i++, k++) memcpy(c + (size_t)k * 8, markers[(size_t)f * cap_per_frame + i].corners, 32);
    }
    first[F] = k;
    return at;
}

fid_status draw_launch_markers(hipStream_t st, uint8_t *img, int W, int H, long long stride, long long fstride, const uint8_t *d_pack, size_t at, int F, uint32_t flags)
{
    const dim3 grid((unsigned)(F < 65536 ? F : 65536)), block(256);
    hipLaunchKernelGGL(k_draw_markers, grid, block, 0, st, img, W, H, stride, fstride, (const float *)(d_pack + at), (const int *)d_pack, F,
                       (flags & FID_DRAW_FIRST_CORNER_LINE8) ? 1 : 0);
    return hipGetLastError() == hipSuccess ? FID_OK : FID_E_HIP;
}

// ---- the two calls on a caller's device memory: where the bytes lie decides the device.  [d, d + span) must be device memory of
// ONE device, inside the allocation around d where the runtime knows it (the check fid_stag_detect_markers_device makes).
int draw_device_of(const uint8_t *d, unsigned long long span)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, d) != hipSuccess) {
        (void)hipGetLastError();  // (not a HIP allocation: the error must not be left for the launches' checks to find)
        return -1;
    }
    if ((a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) || !stag_on_device(d + span - 1, a.device)) return -1;
    hipDeviceptr_t base = nullptr;
    size_t bytes = 0;
    if (hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)d) == hipSuccess) {
        if (d + span > (const uint8_t *)base + bytes) return -1;
    } else {
        (void)hipGetLastError();
    }
    return a.device;
}

// a stream and a marker buffer per device, made on first use and kept for the process (never freed: the runtime may be gone when
// static destructors run).  One call per device at a time.
struct DrawDevice {
    std::mutex m;
    hipStream_t stream = nullptr;
    uint8_t *d_pack = nullptr;
    size_t cap = 0;
};
DrawDevice *draw_device(int dev)
{
    static std::mutex g;
    static std::vector<DrawDevice *> all;
    std::lock_guard<std::mutex> lk(g);
    if ((size_t)dev >= all.size()) all.resize((size_t)dev + 1, nullptr);
    if (!all[(size_t)dev]) all[(size_t)dev] = new DrawDevice();
    return all[(size_t)dev];
}

// the calling thread's current device is put back when the call returns (a torch caller keeps its own)
struct DrawDeviceScope {
    int prev = -1;
    hipError_t rc;
    explicit DrawDeviceScope(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        rc = hipSetDevice(dev);
    }
    ~DrawDeviceScope()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

fid_status draw_hip(hipError_t e) { return e == hipSuccess ? FID_OK : (e == hipErrorOutOfMemory ? FID_E_OUT_OF_MEMORY : FID_E_HIP); }

}  // namespace

extern "C" {

fid_status fid_to_bgr_device(const void *d_src, int32_t nframes, int32_t width, int32_t height, int32_t stride, int64_t frame_stride, fid_encoding enc,
                             void *d_bgr, int32_t bgr_stride, int64_t bgr_frame_stride)
{
    if (!d_src || !d_bgr || nframes < 1 || width < 1 || height < 1) return FID_E_INVALID_ARG;
    const int bpp = draw_enc_bpp(enc);
    if (bpp == 0 || (int64_t)stride < (int64_t)width * bpp || (int64_t)bgr_stride < (int64_t)width * 3) return FID_E_INVALID_ARG;
    const int64_t sframe = (int64_t)(height - 1) * stride + (int64_t)width * bpp, dframe = (int64_t)(height - 1) * bgr_stride + (int64_t)width * 3;
    if (nframes > 1 && (frame_stride < 0 || bgr_frame_stride < dframe)) return FID_E_INVALID_ARG;  // (the frames written must not overlap)
    const int64_t sfs = nframes > 1 ? frame_stride : 0, dfs = nframes > 1 ? bgr_frame_stride : 0;
    const unsigned long long sspan = (unsigned long long)(nframes - 1) * (unsigned long long)sfs + (unsigned long long)sframe;
    const unsigned long long dspan = (unsigned long long)(nframes - 1) * (unsigned long long)dfs + (unsigned long long)dframe;
    const uint8_t *s = (const uint8_t *)d_src;
    uint8_t *d = (uint8_t *)d_bgr;
    if (s < d + dspan && d < s + sspan) return FID_E_INVALID_ARG;  // (in place, or overlapping: not a copy)
    const int dev = draw_device_of(s, sspan);
    if (dev < 0 || draw_device_of(d, dspan) != dev) return FID_E_INVALID_ARG;
    DrawDevice *dd = draw_device(dev);
    std::lock_guard<std::mutex> lk(dd->m);
    DrawDeviceScope scope(dev);
    if (scope.rc != hipSuccess) return FID_E_HIP;
    if (!dd->stream && hipStreamCreateWithFlags(&dd->stream, hipStreamNonBlocking) != hipSuccess) return FID_E_HIP;
    const fid_status rc = draw_launch_to_bgr(dd->stream, s, stride, sfs, enc, d, bgr_stride, dfs, width, height, nframes);
    if (rc != FID_OK) return rc;
    return draw_hip(hipStreamSynchronize(dd->stream));
}

fid_status fid_draw_detected_markers_device(void *d_bgr, int32_t nframes, int32_t width, int32_t height, int32_t stride, int64_t frame_stride,
                                            const fid_marker *markers, int32_t cap_per_frame, const int32_t *n_per_frame, uint32_t flags)
{
    if (!d_bgr || !n_per_frame || nframes < 1 || width < 1 || height < 1 || (int64_t)stride < (int64_t)width * 3) return FID_E_INVALID_ARG;
    if ((flags & ~(uint32_t)FID_DRAW_FIRST_CORNER_LINE8) || cap_per_frame < 0 || cap_per_frame > kDrawMaxMarkers) return FID_E_INVALID_ARG;
    const int64_t frame = (int64_t)(height - 1) * stride + (int64_t)width * 3;
    if (nframes > 1 && frame_stride < frame) return FID_E_INVALID_ARG;  // (the frames drawn on must not overlap)
    int64_t total = 0;
    for (int f = 0; f < nframes; f++) {
        if (n_per_frame[f] < 0 || n_per_frame[f] > cap_per_frame) return FID_E_INVALID_ARG;
        total += n_per_frame[f];
    }
    if (total > 0 && !markers) return FID_E_INVALID_ARG;
    const int64_t fs = nframes > 1 ? frame_stride : 0;
    const unsigned long long span = (unsigned long long)(nframes - 1) * (unsigned long long)fs + (unsigned long long)frame;
    const int dev = draw_device_of((const uint8_t *)d_bgr, span);
    if (dev < 0) return FID_E_INVALID_ARG;
    if (total == 0) return FID_OK;
    std::vector<uint8_t> pack;
    const size_t at = draw_pack(markers, cap_per_frame, n_per_frame, nframes, &pack);
    DrawDevice *dd = draw_device(dev);
    std::lock_guard<std::mutex> lk(dd->m);
    DrawDeviceScope scope(dev);
    if (scope.rc != hipSuccess) return FID_E_HIP;
    if (!dd->stream && hipStreamCreateWithFlags(&dd->stream, hipStreamNonBlocking) != hipSuccess) return FID_E_HIP;
    if (pack.size() > dd->cap) {
        if (dd->d_pack) (void)hipFree(dd->d_pack);
        dd->d_pack = nullptr;
        dd->cap = 0;
        const fid_status rca = draw_hip(hipMalloc((void **)&dd->d_pack, pack.size()));
        if (rca != FID_OK) return rca;
        dd->cap = pack.size();
    }
    fid_status rc = draw_hip(hipMemcpyAsync(dd->d_pack, pack.data(), pack.size(), hipMemcpyHostToDevice, dd->stream));
    if (rc == FID_OK) rc = draw_launch_markers(dd->stream, (uint8_t *)d_bgr, width, height, stride, fs, dd->d_pack, at, nframes, flags);
    const fid_status rcs = draw_hip(hipStreamSynchronize(dd->stream));  // (the packed markers live until the copy is done)
    return rc != FID_OK ? rc : rcs;
}

fid_status fid_jpeg_marker_image(fid_jpeg_ctx *c, int32_t frame, fid_encoding base, const fid_marker *markers, int32_t n, uint32_t flags,
                                 uint8_t *host_bgr, int64_t host_bytes)
{
    if (!c || !host_bgr || n < 0 || n > kDrawMaxMarkers || (n > 0 && !markers) || (flags & ~(uint32_t)FID_DRAW_FIRST_CORNER_LINE8)) return FID_E_INVALID_ARG;
    if (base != FID_ENC_BGR8 && base != FID_ENC_MONO8) return FID_E_INVALID_ARG;
    if (c->last_n <= 0 || frame < 0 || frame >= c->last_n) {
        c->last_error = "fid_jpeg_marker_image: no such frame in the last decode";
        return FID_E_INVALID_ARG;
    }
    if ((int)base != c->last_enc) {
        c->last_error = "fid_jpeg_marker_image: the last decode made the other image (BGR8 / MONO8)";
        return FID_E_INVALID_ARG;
    }
    const int W = c->last_w, H = c->last_h, bpp = base == FID_ENC_MONO8 ? 1 : 3;
    const int64_t bytes = (int64_t)W * H * 3;
    if (host_bytes < bytes) return FID_E_CAPACITY;
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
    if (rc == FID_OK) JPCHK(c, hipMemcpyAsync(host_bgr, c->d_mark, (size_t)bytes, hipMemcpyDeviceToHost, st));
    JPCHK(c, hipStreamSynchronize(st));
    if (rc != FID_OK) c->last_error = "fid_jpeg_marker_image: a kernel launch failed";
    return rc;
}

}  // extern "C"
