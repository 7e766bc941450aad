// CharucoBoard (host/include/charuco_board.hpp): a frame -> fid_detect -> the chessboard corners of the last call, the same from the
// markers and the image handed back in, the board pose over them, and what the caller recorded for the same frame.
//   usage: charuco_test <frame.pgm> <case.txt> <data dir>
// case.txt (tests/test_gpu_charuco_host.py writes it from tests/charuco_cases.py):
//   dictionary squares_x squares_y square_len marker_len first_id
//   fx fy cx cy k1 k2 p1 p2 k3
//   n, then per corner the caller found with the camera: id x y (floats printed to nine digits: they read back bit for bit)
//   tvec of the caller's pose (3)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "charuco_board.hpp"
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

static bool same(const std::vector<fid_charuco_corner> &a, const std::vector<fid_charuco_corner> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(fid_charuco_corner)) == 0);
}

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
    int dicno = 0, sx = 0, sy = 0, first_id = 0, n_want = 0;
    double sl = 0, ml = 0, want_t[3] = {0, 0, 0};
    fid_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.model = FID_CAM_PLUMB_BOB;
    cam.n_dist = 5;
    cam.K[8] = 1.;
    in >> dicno >> sx >> sy >> sl >> ml >> first_id;
    in >> cam.K[0] >> cam.K[4] >> cam.K[2] >> cam.K[5];
    for (int i = 0; i < 5; i++) in >> cam.D[i];
    in >> n_want;
    std::vector<fid_charuco_corner> want((size_t)(n_want > 0 ? n_want : 0));
    for (fid_charuco_corner &c : want) in >> c.id >> c.x >> c.y;
    for (double &t : want_t) in >> t;
    CHECK(bool(in) && n_want >= 4);
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
        CharucoBoard board(ctx);
        std::vector<std::vector<fid_charuco_corner>> last;
        CHECK(board.corners() == 0 && board.interpolateLast(nullptr, 1, &last) == FID_E_INVALID_ARG);  // no board yet
        CHECK(board.create(1, sy, sl, ml, first_id) == FID_E_INVALID_ARG && std::strstr(fid_last_error(ctx), "at least 2") != nullptr);
        CHECK(board.create(sx, sy, sl, ml, first_id) == FID_OK);
        CHECK(board.corners() == (sx - 1) * (sy - 1) && board.markers() == sx * sy / 2);

        std::vector<fid_marker> markers(256);
        int32_t n = 0;
        CHECK(fid_detect(ctx, pix.data(), W, H, W, FID_ENC_MONO8, markers.data(), (int32_t)markers.size(), &n) == FID_OK);
        markers.resize((size_t)(n > 0 ? n : 0));
        std::printf("%d markers\n", n);

        // the corners of the last call, by either route, and the same from the markers and the image handed back in
        std::vector<std::vector<fid_charuco_corner>> hom, viaCam;
        CHECK(board.interpolateLast(nullptr, 1, &hom) == FID_OK && board.interpolateLast(&cam, 1, &viaCam) == FID_OK);
        std::vector<fid_charuco_corner> homHost, camHost;
        CHECK(board.interpolate(nullptr, markers, pix.data(), W, H, W, &homHost) == FID_OK && same(hom[0], homHost));
        CHECK(board.interpolate(&cam, markers, pix.data(), W, H, W, &camHost) == FID_OK && same(viaCam[0], camHost));
        CHECK(camHost.size() == want.size());
        for (size_t i = 0; i < camHost.size() && i < want.size(); i++)
            CHECK(camHost[i].id == want[i].id && camHost[i].x == want[i].x && camHost[i].y == want[i].y);
        for (const fid_charuco_corner &c : homHost) CHECK(c.win >= 1 && c.win <= 10 && std::fabs(c.x - c.x0) <= c.win && std::fabs(c.y - c.y0) <= c.win);

        // the pose: of the last call, and of the corners held here
        std::vector<fid_charuco_pose_out> poses;
        fid_charuco_pose_out one;
        CHECK(board.poseLast(cam, 1, &poses) == FID_OK && poses.size() == 1 && board.pose(cam, camHost, &one) == FID_OK);
        CHECK(poses.size() == 1 && std::memcmp(&poses[0], &one, sizeof(one)) == 0);
        CHECK(one.status == FID_CHARUCO_POSE_OK && one.n_corners == (int)camHost.size());
        for (int a = 0; a < 3; a++) CHECK(one.tvec[a] == want_t[a]);
        std::printf("%d corners, board at %.4f %.4f %.4f, mean squared error %.4f px^2\n", one.n_corners, one.tvec[0], one.tvec[1], one.tvec[2], one.image_error);
        // the first corner reprojects within 3 px of where it was refined (the pinhole part only: the check is coarse on purpose)
        double p[3];
        board.objectPoint(camHost.empty() ? 0 : camHost[0].id, p);
        const double Xc[3] = {one.R[0] * p[0] + one.R[1] * p[1] + one.tvec[0], one.R[3] * p[0] + one.R[4] * p[1] + one.tvec[1],
                              one.R[6] * p[0] + one.R[7] * p[1] + one.tvec[2]};
        if (!camHost.empty()) {
            CHECK(std::fabs(cam.K[0] * Xc[0] / Xc[2] + cam.K[2] - camHost[0].x) < 3. && std::fabs(cam.K[4] * Xc[1] / Xc[2] + cam.K[5] - camHost[0].y) < 3.);
        }
        // three corners: no pose, and the record says why
        std::vector<fid_charuco_corner> three(camHost.begin(), camHost.begin() + (camHost.size() >= 3 ? 3 : 0));
        CHECK(board.pose(cam, three, &one) == FID_OK && one.status == FID_CHARUCO_POSE_FEW && one.n_corners == 3 && one.tvec[2] == 0.);
    }
    // the board left with its wrapper
    fid_charuco_corner c;
    int32_t n = 0;
    CHECK(fid_charuco_last_cam(ctx, nullptr, 2, &c, 1, &n) == FID_E_INVALID_ARG && std::strstr(fid_last_error(ctx), "no ChArUco board") != nullptr);
    fid_destroy(ctx);
    if (g_fail) return 1;
    std::printf("all checks passed\n");
    return 0;
}
