// compressed_out_test.cpp -- what the two nodes publish on <marker image topic>/compressed for a COMPRESSED frame:
//   usage: compressed_out_test <dir> <data_dir>
// <dir> holds what tests/test_gpu_compressed_out_host.py writes: tag_01 as a colour 4:2:0 JPEG and as a colour PNG, a frame without
// markers as JPEG, and an HD21 STag frame as JPEG and PNG.  compressedImageCallback(msg, out, CompressedImage *) must publish
// "bgr8; jpeg compressed bgr8" with the source header, and its data must be, byte for byte, the file the device encoder makes
// (fid_jpeg_encode, quality 80, 4:2:0) of the raw marker image the Image overload publishes for the same frame -- which
// tests/test_gpu_marker_jpeg.py pins on libjpeg-turbo's file.  Nothing with the option off or for a damaged frame; the vertices and
// markers are those of the other overloads.
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

static bool isPng(const std::vector<uint8_t> &d) { return d.size() >= 8 && d[0] == 0x89 && d[1] == 'P' && d[2] == 'N' && d[3] == 'G'; }
static bool sameHeader(const Header &a, const Header &b) { return a.seq == b.seq && a.sec == b.sec && a.nsec == b.nsec && a.frame_id == b.frame_id; }

static Header testHeader(uint32_t seq)
{
    Header h;
    h.seq = seq;
    h.sec = 1491682360;
    h.nsec = 314066469;
    h.frame_id = "raspicam";
    return h;
}

// the file of a raw BGR8 marker image at the encoder's defaults
static std::vector<uint8_t> encodeRaw(const Image &img)
{
    fid_jpeg_enc_ctx *e = nullptr;
    if (fid_jpeg_enc_create(0, (int32_t)img.width, (int32_t)img.height, 1, 0, &e) != FID_OK) throw std::runtime_error("encoder create");
    std::vector<uint8_t> out((size_t)img.width * img.height * 3 + 65536);
    int64_t nb = 0;
    const fid_status rc = fid_jpeg_encode(e, img.data.data(), 1, (int32_t)img.width, (int32_t)img.height, (int32_t)img.step, 0, FID_ENC_BGR8, out.data(),
                                          (int64_t)out.size(), &nb);
    fid_jpeg_enc_destroy(e);
    if (rc != FID_OK) throw std::runtime_error("encode");
    out.resize((size_t)nb);
    return out;
}

static void checkFile(const CompressedImage &c, const Header &h, const Image &raw)
{
    CHECK(sameHeader(c.header, h) && c.format == "bgr8; jpeg compressed bgr8");
    CHECK(c.data.size() > 623 + 2 && c.data[0] == 0xFF && c.data[1] == 0xD8 && c.data[c.data.size() - 2] == 0xFF && c.data.back() == 0xD9);
    fid_jpeg_info ji = {};
    CHECK(fid_jpeg_probe(c.data.data(), (int64_t)c.data.size(), &ji) == FID_OK);
    CHECK(ji.width == (int32_t)raw.width && ji.height == (int32_t)raw.height && ji.components == 3 && ji.h_samp == 2 && ji.v_samp == 2);
    CHECK(c.data.size() * 4 < raw.data.size());  // (what crosses the link: a fraction of the raw image)
    CHECK(c.data == encodeRaw(raw));
}

static void arucoFrame(const std::string &dir, const std::string &data, const std::string &name, size_t expect_markers)
{
    std::printf("aruco %s\n", name.c_str());
    const std::vector<uint8_t> file = readFile(dir + "/" + name);
    CompressedImage cm;
    cm.header = testHeader(11);
    cm.format = isPng(file) ? "bgr8; png compressed bgr8" : "bgr8; jpeg compressed bgr8";
    cm.data = file;
    FiducialsNode::Params p;
    p.dictionary = 7;
    p.fiducial_len = 0.145;
    p.data_dir = data;
    p.max_width = 1280;
    p.max_height = 960;
    p.publish_images = true;
    FiducialsNode::Params q = p;
    q.publish_images = false;
    FiducialsNode on(p), off(q);
    FiducialArray a, b, c;
    Image raw;
    CompressedImage out, none;
    none.data.assign(5, 1);
    CHECK(on.compressedImageCallback(cm, &a, &raw) && !raw.data.empty());
    CHECK(on.compressedImageCallback(cm, &b, &out));
    CHECK(off.compressedImageCallback(cm, &c, &none) && none.data.empty());  // the option off: no image
    CHECK(on.compressedImageCallback(cm, &c, nullptr));                      // no image asked for (the existing form still resolves)
    CHECK(a.fiducials.size() == expect_markers && b.fiducials.size() == expect_markers && c.fiducials.size() == expect_markers);
    for (size_t i = 0; i < a.fiducials.size() && i < b.fiducials.size(); i++)
        CHECK(a.fiducials[i].fiducial_id == b.fiducials[i].fiducial_id && a.fiducials[i].x0 == b.fiducials[i].x0 && a.fiducials[i].y2 == b.fiducials[i].y2);
    checkFile(out, cm.header, raw);
    for (int k = 0; k < 2; k++) {  // frame after frame on the same contexts
        CompressedImage again;
        CHECK(on.compressedImageCallback(cm, &b, &again) && again.data == out.data);
    }
    CompressedImage bad = cm;
    bad.data.resize(bad.data.size() / 2);
    if (!isPng(file)) bad.data.assign(64, 0x41);
    out.data.assign(3, 7);
    CHECK(!on.compressedImageCallback(bad, &a, &out) && out.data.empty() && !on.lastError().empty());
}

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
    Image raw;
    CompressedImage out, none;
    none.data.assign(5, 1);
    CHECK(!node.compressedImageCallback(cm, &o, &out) && out.data.empty());  // no CameraInfo yet: nothing is published
    node.cameraInfoCallback(ci);
    quiet.cameraInfoCallback(ci);
    CHECK(node.compressedImageCallback(cm, &o, &raw) && !raw.data.empty());
    CHECK(node.compressedImageCallback(cm, &o2, &out) && o2.markers.size() == o.markers.size() && o.markers.size() >= 3);
    CHECK(quiet.compressedImageCallback(cm, &o3, &none) && none.data.empty());  // show_markers off: no image
    CHECK(node.compressedImageCallback(cm, &o3, nullptr) && o3.markers.size() == o.markers.size());
    checkFile(out, cm.header, raw);
    CompressedImage bad = cm;
    bad.data.resize(bad.data.size() / 2);
    if (!isPng(file)) bad.data.assign(64, 0x41);
    CHECK(!node.compressedImageCallback(bad, &o, &out) && out.data.empty());
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::printf("usage: %s <dir> <data dir>\n", argv[0]);
        return 2;
    }
    try {
        const std::string dir = argv[1], data = argv[2];
        for (const char *f : {"tag_01_color.jpg", "tag_01_color.png"}) arucoFrame(dir, data, f, 1);
        arucoFrame(dir, data, "blank.jpg", 0);
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
