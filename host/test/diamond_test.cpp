// DiamondDetector (host/include/diamond_detector.hpp): a frame -> fid_detect -> the diamonds of the last call, the same from the markers
// and the image handed back in, their poses, and what the caller recorded for the same frame.
//   usage: diamond_test <frame.pgm> <case.txt> <data dir>
// case.txt (tests/test_gpu_diamond_host.py writes it from tests/diamond_cases.py):
//   dictionary square_marker_rate square_len
//   fx fy cx cy k1 k2 p1 p2 k3
//   n, then per diamond the caller found: four ids, eight corner coordinates (floats printed to nine digits: they read back bit for
//   bit), the tvec of its pose (3)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "diamond_detector.hpp"
#include "fiducials_host.hpp"

using namespace fiducials_amd;

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

static bool readPgm(const char *path, std::vector<uint8_t> *pix, int *w, int *h)
{
    std::ifstream in(path, std::ios::binary);
    std::string magic;
    int maxv = 0;
    in >> magic >> *w >> *h >> maxv;
    if (!in || magic != "P5" || maxv != 255 || *w < 1 || *h < 1) return false;
    in.get();
    pix->resize((size_t)*w * *h);
    in.read((char *)pix->data(), (std::streamsize)pix->size());
    return bool(in);
}

static bool same(const std::vector<fid_diamond> &a, const std::vector<fid_diamond> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(fid_diamond)) == 0);
}

struct Want {
    int ids[4];
    float corners[8];
    double tvec[3];
};

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::printf("usage: %s <frame.pgm> <case.txt> <data dir>\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> pix;
    int W = 0, H = 0;
    CHECK(readPgm(argv[1], &pix, &W, &H));
    std::ifstream in(argv[2]);
    int dicno = 0, n_want = 0;
    double rate = 0, square_len = 0;
    fid_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.model = FID_CAM_PLUMB_BOB;
    cam.n_dist = 5;
    cam.K[8] = 1.;
    in >> dicno >> rate >> square_len;
    in >> cam.K[0] >> cam.K[4] >> cam.K[2] >> cam.K[5];
    for (int i = 0; i < 5; i++) in >> cam.D[i];
    in >> n_want;
    std::vector<Want> want((size_t)(n_want > 0 ? n_want : 0));
    for (Want &w : want) {
        for (int &i : w.ids) in >> i;
        for (float &c : w.corners) in >> c;
        for (double &t : w.tvec) in >> t;
    }
    CHECK(bool(in) && n_want >= 1);
    if (g_fail) return 1;

    Dictionary dict = getPredefinedDictionary(dicno, argv[3]);
    fid_dict fd = dict.view();
    fid_params params;
    fid_default_params(&params);
    fid_limits lim;
    fid_default_limits(&lim);
    lim.max_width = W; lim.max_height = H; lim.max_batch = 1;
    fid_ctx *ctx = nullptr;
    CHECK(fid_create(&params, &fd, &lim, 0, &ctx) == FID_OK);
    if (!ctx) return 1;
    {
        DiamondDetector dd(ctx, rate);
        std::vector<std::vector<fid_diamond>> last;
        CHECK(dd.detectLast(1, &last) == FID_E_INVALID_ARG && std::strstr(fid_last_error(ctx), "no last call") != nullptr);

        std::vector<fid_marker> markers(256);
        int32_t n = 0;
        CHECK(fid_detect(ctx, pix.data(), W, H, W, FID_ENC_MONO8, markers.data(), (int32_t)markers.size(), &n) == FID_OK);
        markers.resize((size_t)(n > 0 ? n : 0));
        std::printf("%d markers\n", n);

        // the diamonds of the last call, and the same from the markers and the image handed back in
        std::vector<fid_diamond> host;
        CHECK(dd.detectLast(1, &last) == FID_OK && last.size() == 1);
        CHECK(dd.detect(markers, pix.data(), W, H, W, &host) == FID_OK && !last.empty() && same(last[0], host));
        CHECK(host.size() == want.size());
        for (size_t i = 0; i < host.size() && i < want.size(); i++) {
            for (int q = 0; q < 4; q++) CHECK(host[i].ids[q] == want[i].ids[q] && host[i].index[q] >= 0 && host[i].index[q] < n);
            for (int q = 0; q < 4; q++) CHECK(markers[(size_t)host[i].index[q]].id == host[i].ids[q]);
            for (int q = 0; q < 8; q++) CHECK(host[i].corners[q] == want[i].corners[q]);
            for (int q = 0; q < 4; q++)
                CHECK(host[i].win[q] >= 1 && host[i].win[q] <= 10 && std::fabs(host[i].corners[2 * q] - host[i].corners0[2 * q]) <= host[i].win[q] &&
                      std::fabs(host[i].corners[2 * q + 1] - host[i].corners0[2 * q + 1]) <= host[i].win[q]);
        }
        // without refinement the corners are the interpolated ones
        dd.options().refine = 0;
        std::vector<fid_diamond> raw;
        CHECK(dd.detect(markers, pix.data(), W, H, W, &raw) == FID_OK && raw.size() == host.size());
        for (size_t i = 0; i < raw.size() && i < host.size(); i++)
            CHECK(std::memcmp(raw[i].corners, raw[i].corners0, sizeof(raw[i].corners)) == 0 && std::memcmp(raw[i].corners0, host[i].corners0, sizeof(raw[i].corners0)) == 0);
        dd.options().refine = 1;

        // the poses: fid_pose_cam's on the equivalent markers
        std::vector<fid_pose_out> poses, direct(host.size());
        CHECK(dd.pose(cam, host, square_len, &poses) == FID_OK && poses.size() == host.size());
        std::vector<fid_marker> eq(host.size());
        std::vector<double> lens(host.size(), square_len);
        for (size_t i = 0; i < host.size(); i++) {
            eq[i].id = host[i].ids[0];
            std::memcpy(eq[i].corners, host[i].corners, sizeof(eq[i].corners));
        }
        CHECK(fid_pose_cam(ctx, &cam, eq.data(), lens.data(), (int32_t)eq.size(), square_len, direct.data()) == FID_OK);
        CHECK(!poses.empty() && std::memcmp(poses.data(), direct.data(), poses.size() * sizeof(fid_pose_out)) == 0);
        for (size_t i = 0; i < poses.size() && i < want.size(); i++) {
            for (int a = 0; a < 3; a++) CHECK(poses[i].tvec[a] == want[i].tvec[a]);
            std::printf("diamond %d,%d,%d,%d at %.4f %.4f %.4f\n", host[i].ids[0], host[i].ids[1], host[i].ids[2], host[i].ids[3], poses[i].tvec[0],
                        poses[i].tvec[1], poses[i].tvec[2]);
        }

        // the refusals name the bound
        dd.options().square_marker_rate = 1.0;
        CHECK(dd.detectLast(1, &last) == FID_E_INVALID_ARG && std::strstr(fid_last_error(ctx), "square_marker_rate") != nullptr);
        dd.options().square_marker_rate = rate;
        dd.options().max_rep_rate = 0.;
        CHECK(dd.detect(markers, pix.data(), W, H, W, &raw) == FID_E_INVALID_ARG && raw.empty() && std::strstr(fid_last_error(ctx), "max_rep_rate") != nullptr);
    }
    fid_destroy(ctx);
    if (g_fail) return 1;
    std::printf("all checks passed\n");
    return 0;
}
