// stag_compressed_test.cpp -- StagNode::compressedImageCallback (host/include/stag_host.hpp) on one frame as JPEG and as PNG:
//   usage: stag_compressed_test <frame.jpg> <frame.png> <data_dir> <hd> <errorCorrection>
// The node must publish for a compressed frame exactly what imageCallback publishes for the mono8 frame the file decodes to (JPEG:
// fid_jpeg_decode to host memory; PNG: fid_png_decode), nothing before the first CameraInfo, and nothing for a damaged file.
#include <cstdio>
#include <fstream>
#include <iterator>

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

static std::vector<uint8_t> readFile(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static bool sameHeader(const Header &a, const Header &b)
{
    return a.seq == b.seq && a.sec == b.sec && a.nsec == b.nsec && a.frame_id == b.frame_id;
}
static bool samePose(const Pose &a, const Pose &b)
{
    return a.px == b.px && a.py == b.py && a.pz == b.pz && a.ox == b.ox && a.oy == b.oy && a.oz == b.oz && a.ow == b.ow;
}
// everything the node publishes, field by field and bit for bit
static bool sameOutputs(const StagNode::Outputs &a, const StagNode::Outputs &b)
{
    if (a.array_published != b.array_published || a.markers.size() != b.markers.size() || a.tf.size() != b.tf.size()) return false;
    if (!sameHeader(a.array.header, b.array.header) || a.array.detections.size() != b.array.detections.size()) return false;
    for (size_t i = 0; i < a.markers.size(); i++)
        if (!sameHeader(a.markers[i].header, b.markers[i].header) || !samePose(a.markers[i].pose, b.markers[i].pose)) return false;
    for (size_t i = 0; i < a.tf.size(); i++) {
        const TransformStamped &s = a.tf[i], &t = b.tf[i];
        if (!sameHeader(s.header, t.header) || s.child_frame_id != t.child_frame_id || s.tx != t.tx || s.ty != t.ty || s.tz != t.tz ||
            s.qx != t.qx || s.qy != t.qy || s.qz != t.qz || s.qw != t.qw)
            return false;
    }
    for (size_t i = 0; i < a.array.detections.size(); i++) {
        const Detection2D &s = a.array.detections[i], &t = b.array.detections[i];
        if (!sameHeader(s.header, t.header) || s.results.size() != t.results.size()) return false;
        for (size_t k = 0; k < s.results.size(); k++)
            if (s.results[k].id != t.results[k].id || s.results[k].score != t.results[k].score || !samePose(s.results[k].pose, t.results[k].pose))
                return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::printf("usage: %s <frame.jpg> <frame.png> <data dir> <hd> <errorCorrection>\n", argv[0]);
        return 2;
    }
    try {
        const std::vector<uint8_t> jpg = readFile(argv[1]), png = readFile(argv[2]);
        Header hdr;
        hdr.seq = 42; hdr.sec = 100; hdr.nsec = 7; hdr.frame_id = "raspicam";
        // what each file decodes to, as the mono8 Image imageCallback would get
        fid_png_info pi = {};
        CHECK(fid_png_probe(png.data(), (int64_t)png.size(), &pi) == FID_OK);
        const int w = pi.width, h = pi.height;
        Image fromPng, fromJpg;
        fromPng.header = fromJpg.header = hdr;
        fromPng.width = fromJpg.width = (uint32_t)w;
        fromPng.height = fromJpg.height = (uint32_t)h;
        fromPng.step = fromJpg.step = (uint32_t)w;
        fromPng.encoding = fromJpg.encoding = "mono8";
        fromPng.data.resize((size_t)w * h);
        CHECK(fid_png_decode(png.data(), (int64_t)png.size(), FID_ENC_MONO8, fromPng.data.data(), (int64_t)fromPng.data.size(), nullptr) == FID_OK);
        {
            fid_jpeg_ctx *j = nullptr;
            CHECK(fid_jpeg_create(0, w, h, 1, &j) == FID_OK);
            fromJpg.data.resize((size_t)w * h);
            const uint8_t *file = jpg.data();
            const int64_t nbytes = (int64_t)jpg.size();
            CHECK(fid_jpeg_decode(j, &file, &nbytes, 1, FID_ENC_MONO8, fromJpg.data.data(), (int64_t)w * h) == FID_OK);
            fid_jpeg_destroy(j);
        }
        StagNode::Params p;
        p.libraryHD = std::atoi(argv[4]);
        p.errorCorrection = std::atoi(argv[5]);
        p.marker_size = 0.14f;
        p.publish_tf = true;
        p.is_compressed = true;
        StagNode node(p, argv[3], w, h);
        CompressedImage cj, cp;
        cj.header = cp.header = hdr;
        cj.format = "jpeg";
        cj.data = jpg;
        cp.format = "mono8; png compressed ";
        cp.data = png;
        StagNode::Outputs got, want;
        CHECK(!node.compressedImageCallback(cj, &got) && got.markers.empty() && !got.array_published);  // no camera info yet
        CameraInfo cam;
        cam.K = {1400.0 * w / 1920, 0, w / 2.0, 0, 1400.0 * w / 1920, h / 2.0, 0, 0, 1};
        cam.D = {0, 0, 0, 0, 0};
        node.cameraInfoCallback(cam);
        // JPEG: decoded on the device and detected where it lies
        CHECK(node.compressedImageCallback(cj, &got));
        CHECK(node.imageCallback(fromJpg, &want));
        CHECK(want.markers.size() >= 3);
        CHECK(sameOutputs(got, want));
        // PNG: decoded on the host
        CHECK(node.compressedImageCallback(cp, &got));
        CHECK(node.imageCallback(fromPng, &want));
        CHECK(want.markers.size() >= 3);
        CHECK(sameOutputs(got, want));
        // and the JPEG again after the PNG (the decoder context is reused)
        CHECK(node.compressedImageCallback(cj, &got) && node.imageCallback(fromJpg, &want) && sameOutputs(got, want));
        // files that cannot be decoded publish nothing: a JPEG cut inside its header, a JPEG without its SOI, a PNG with a broken chunk,
        // garbage, nothing.  (A JPEG cut inside its scan data is not among them: libjpeg decodes it with a warning and fills the rest,
        // and cv::imdecode returns that image.)
        std::vector<std::vector<uint8_t>> bad;
        bad.push_back(std::vector<uint8_t>(jpg.begin(), jpg.begin() + 100));
        bad.push_back(std::vector<uint8_t>(jpg.begin() + 2, jpg.end()));
        {
            std::vector<uint8_t> b = png;
            for (size_t k = png.size() / 2; k < png.size() / 2 + 64 && k < b.size(); k++) b[k] ^= 0x5a;
            bad.push_back(b);
        }
        bad.push_back(std::vector<uint8_t>(4096, 0x17));
        bad.push_back(std::vector<uint8_t>());
        for (size_t k = 0; k < bad.size(); k++) {
            CompressedImage cb = cj;
            cb.data = bad[k];
            StagNode::Outputs o;
            o.array_published = true;
            const bool published = node.compressedImageCallback(cb, &o);
            if (published) std::printf("damaged file %zu was published\n", k);
            CHECK(!published && o.markers.empty() && o.tf.empty() && !o.array_published);
            CHECK(!node.lastError().empty());
        }
        // the node still serves a good frame after them
        CHECK(node.compressedImageCallback(cj, &got) && node.imageCallback(fromJpg, &want) && sameOutputs(got, want));
    } catch (const std::exception &e) {
        std::printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    std::printf(g_fail ? "%d check(s) failed\n" : "all checks passed%.0d\n", g_fail);
    return g_fail ? 1 : 0;
}
