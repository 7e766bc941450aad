// marker_images_test.cpp -- the marker images the two nodes publish for a COMPRESSED frame (the shipped launch defaults):
//   usage: marker_images_test <dir> <data_dir>
// <dir> holds what tests/test_gpu_marker_images_host.py writes: tag_01.pgm (the reference's test image), tag_01 as a one-component
// JPEG, as a colour 4:2:0 JPEG and as gray / colour PNGs, a frame without markers as JPEG and PNG, and an HD21 STag frame as JPEG
// and PNG.  FiducialsNode::compressedImageCallback(msg, out, image) must publish the decoded BGR8 frame with the outlines the host
// drawer puts on it (nothing drawn when nothing was found) and the vertices of the image-less call; StagNode's must publish the
// detector's gray image expanded to BGR with the host drawer's outlines.  Nothing with the option off or for a damaged file.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>

#include "fiducials_host.hpp"
#include "stag_host.hpp"

using namespace fiducials_amd;

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

static std::vector<uint8_t> readFile(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read " + path);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static Image loadPgm(const std::string &path, const Header &h)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::string magic;
    int w, ht, maxv;
    f >> magic >> w >> ht >> maxv;
    f.get();
    Image im;
    im.header = h;
    im.width = (uint32_t)w;
    im.height = (uint32_t)ht;
    im.encoding = "mono8";
    im.step = (uint32_t)w;
    im.data.resize((size_t)w * ht);
    f.read((char *)im.data.data(), (std::streamsize)im.data.size());
    return im;
}

static bool isPng(const std::vector<uint8_t> &d) { return d.size() >= 8 && d[0] == 0x89 && d[1] == 'P' && d[2] == 'N' && d[3] == 'G'; }

// what the subscriber plugin's cv::imdecode hands over, made with the library's own decoders into host memory: BGR8 or MONO8
static std::vector<uint8_t> decodeOnHost(const std::vector<uint8_t> &file, fid_encoding enc, int *w, int *h)
{
    const int px = enc == FID_ENC_MONO8 ? 1 : 3;
    std::vector<uint8_t> out;
    if (isPng(file)) {
        fid_png_info pi = {};
        if (fid_png_probe(file.data(), (int64_t)file.size(), &pi) != FID_OK) throw std::runtime_error("png probe");
        *w = pi.width;
        *h = pi.height;
        out.resize((size_t)pi.width * pi.height * px);
        if (fid_png_decode(file.data(), (int64_t)file.size(), enc, out.data(), (int64_t)out.size(), nullptr) != FID_OK) throw std::runtime_error("png decode");
        return out;
    }
    fid_jpeg_info ji = {};
    if (fid_jpeg_probe(file.data(), (int64_t)file.size(), &ji) != FID_OK) throw std::runtime_error("jpeg probe");
    *w = ji.width;
    *h = ji.height;
    out.resize((size_t)ji.width * ji.height * px);
    fid_jpeg_ctx *j = nullptr;
    if (fid_jpeg_create(0, ji.width, ji.height, 1, &j) != FID_OK) throw std::runtime_error("jpeg create");
    const uint8_t *p = file.data();
    const int64_t n = (int64_t)file.size();
    const fid_status rc = fid_jpeg_decode(j, &p, &n, 1, enc, out.data(), (int64_t)out.size());
    fid_jpeg_destroy(j);
    if (rc != FID_OK) throw std::runtime_error("jpeg decode");
    return out;
}

static bool sameVertices(const FiducialArray &a, const FiducialArray &b)
{
    if (a.image_seq != b.image_seq || a.fiducials.size() != b.fiducials.size()) return false;
    for (size_t i = 0; i < a.fiducials.size(); i++) {
        const Fiducial &p = a.fiducials[i], &q = b.fiducials[i];
        if (p.fiducial_id != q.fiducial_id || p.x0 != q.x0 || p.y0 != q.y0 || p.x1 != q.x1 || p.y1 != q.y1 || p.x2 != q.x2 || p.y2 != q.y2 ||
            p.x3 != q.x3 || p.y3 != q.y3)
            return false;
    }
    return true;
}

static bool sameHeader(const Header &a, const Header &b) { return a.seq == b.seq && a.sec == b.sec && a.nsec == b.nsec && a.frame_id == b.frame_id; }

static bool isMarkerImageOf(const Image &img, const Header &h, int w, int ht)
{
    return sameHeader(img.header, h) && img.encoding == "bgr8" && img.is_bigendian == 0 && (int)img.width == w && (int)img.height == ht &&
           img.step == (uint32_t)w * 3 && img.data.size() == (size_t)w * ht * 3;
}

static Header testHeader(uint32_t seq)
{
    Header h;
    h.seq = seq;
    h.sec = 1491682360;
    h.nsec = 314066469;
    h.frame_id = "raspicam";
    return h;
}

static FiducialsNode::Params arucoParams(const std::string &data, bool publish_images)
{
    FiducialsNode::Params p;
    p.dictionary = 7;  // aruco_images.test
    p.fiducial_len = 0.145;
    p.data_dir = data;
    p.max_width = 1280;
    p.max_height = 960;
    p.publish_images = publish_images;
    return p;
}

// one compressed frame through FiducialsNode with ~publish_images on and off
static void arucoFrame(const std::string &dir, const std::string &data, const std::string &name, size_t expect_markers)
{
    std::printf("aruco %s\n", name.c_str());
    const std::vector<uint8_t> file = readFile(dir + "/" + name);
    CompressedImage cm;
    cm.header = testHeader(11);
    cm.format = isPng(file) ? "bgr8; png compressed bgr8" : "bgr8; jpeg compressed bgr8";
    cm.data = file;
    FiducialsNode on(arucoParams(data, true)), off(arucoParams(data, false));
    FiducialArray a, b, c;
    Image img, none;
    none.data.assign(5, 1);
    CHECK(on.compressedImageCallback(cm, &a, &img));
    CHECK(off.compressedImageCallback(cm, &b, &none) && none.data.empty());  // the option off: no image
    CHECK(off.compressedImageCallback(cm, &c));
    CHECK(on.compressedImageCallback(cm, &c, nullptr));                      // no image asked for
    CHECK(sameVertices(a, b) && sameVertices(a, c));  // the BGR8 road detects on the same 15-bit gray as the MONO8 one
    CHECK(a.image_seq == 11 && a.fiducials.size() == expect_markers);
    int w = 0, h = 0;
    std::vector<uint8_t> want = decodeOnHost(file, FID_ENC_BGR8, &w, &h);
    if (!a.fiducials.empty()) {
        std::vector<fid_marker> mk;
        for (const Fiducial &f : a.fiducials) {
            fid_marker m;
            m.id = f.fiducial_id;
            const double v[8] = {f.x0, f.y0, f.x1, f.y1, f.x2, f.y2, f.x3, f.y3};
            for (int k = 0; k < 8; k++) m.corners[k] = (float)v[k];
            mk.push_back(m);
        }
        CHECK(fid_draw_detected_markers(want.data(), w, h, w * 3, mk.data(), (int32_t)mk.size(), 0) == FID_OK);
    }
    CHECK(isMarkerImageOf(img, cm.header, w, h));
    CHECK(img.data == want);
    // the same frame through the raw road: the same message fields
    if (w == 1280 && h == 960) {
        FiducialArray r;
        Image raw;
        CHECK(on.imageCallback(loadPgm(dir + "/tag_01.pgm", cm.header), &r, &raw));
        CHECK(sameHeader(raw.header, img.header) && raw.encoding == img.encoding && raw.step == img.step && raw.width == img.width &&
              raw.height == img.height && raw.data.size() == img.data.size() && raw.is_bigendian == img.is_bigendian);
    }
    // a frame that cannot be decoded: nothing, no image
    CompressedImage bad = cm;
    bad.data.resize(bad.data.size() / 2);
    if (!isPng(file)) bad.data.assign(64, 0x41);
    img.data.assign(3, 7);
    CHECK(!on.compressedImageCallback(bad, &a, &img) && img.data.empty() && !on.lastError().empty());
    // ... and the node goes on with the next good frame
    CHECK(on.compressedImageCallback(cm, &a, &img) && img.data == want);
}

// one compressed frame through StagNode with show_markers on and off
static void stagFrame(const std::string &dir, const std::string &data, const std::string &name)
{
    std::printf("stag %s\n", name.c_str());
    const std::vector<uint8_t> file = readFile(dir + "/" + name);
    CompressedImage cm;
    cm.header = testHeader(21);
    cm.format = isPng(file) ? "mono8; png compressed mono8" : "mono8; jpeg compressed mono8";
    cm.data = file;
    CameraInfo ci;
    ci.K = {933.3, 0, 640, 0, 933.3, 360, 0, 0, 1};
    ci.D = {0, 0, 0, 0, 0};
    ci.header.frame_id = "camera";
    StagNode::Params p;
    p.libraryHD = 21;
    p.errorCorrection = 7;
    StagNode::Params q = p;
    q.show_markers = false;
    StagNode node(p, data, 1280, 720), quiet(q, data, 1280, 720);
    StagNode::Outputs o, o2, o3;
    Image img, none;
    CHECK(!node.compressedImageCallback(cm, &o, &img) && img.data.empty());  // no CameraInfo yet: nothing is published
    node.cameraInfoCallback(ci);
    quiet.cameraInfoCallback(ci);
    CHECK(node.compressedImageCallback(cm, &o, &img));
    const std::vector<Marker> markers = node.lastMarkers();
    CHECK(markers.size() >= 3 && o.markers.size() == markers.size());
    CHECK(quiet.compressedImageCallback(cm, &o2, &none) && none.data.empty());  // show_markers off: no image
    CHECK(node.compressedImageCallback(cm, &o3) && o3.markers.size() == o.markers.size());
    for (size_t i = 0; i < o.markers.size() && i < o2.markers.size(); i++) CHECK(o.markers[i].pose.px == o2.markers[i].pose.px);
    int w = 0, h = 0;
    const std::vector<uint8_t> gray = decodeOnHost(file, FID_ENC_MONO8, &w, &h);
    std::vector<uint8_t> want((size_t)w * h * 3);
    CHECK(fid_to_bgr(gray.data(), w, h, w, FID_ENC_MONO8, want.data(), (int64_t)want.size()) == FID_OK);
    std::vector<fid_marker> mk;
    for (const Marker &m : markers) {
        fid_marker k;
        k.id = m.id;
        for (int c = 0; c < 4; c++) {
            k.corners[2 * c] = (float)m.corners[(size_t)c].x;
            k.corners[2 * c + 1] = (float)m.corners[(size_t)c].y;
        }
        mk.push_back(k);
    }
    CHECK(fid_draw_detected_markers(want.data(), w, h, w * 3, mk.data(), (int32_t)mk.size(), 0) == FID_OK);
    CHECK(isMarkerImageOf(img, cm.header, w, h));
    CHECK(img.data == want);
    CompressedImage bad = cm;
    bad.data.resize(bad.data.size() / 2);
    if (!isPng(file)) bad.data.assign(64, 0x41);
    CHECK(!node.compressedImageCallback(bad, &o, &img) && img.data.empty());
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::printf("usage: %s <dir> <data dir>\n", argv[0]);
        return 2;
    }
    try {
        const std::string dir = argv[1], data = argv[2];
        for (const char *f : {"tag_01_gray.jpg", "tag_01_color.jpg", "tag_01_gray.png", "tag_01_color.png"}) arucoFrame(dir, data, f, 1);
        for (const char *f : {"blank.jpg", "blank.png"}) arucoFrame(dir, data, f, 0);
        for (const char *f : {"stag.jpg", "stag.png"}) stagFrame(dir, data, f);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception %s\n", e.what());
        return 1;
    }
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
