// CharucoCalibrator (host/include/camera_calibrator.hpp): views of chessboard corner records -> calibrate -> CameraInfo -> YAML -> read
// back -> fid_camera_from_info gives the same camera.
//   usage: charuco_calibrate_test <views.txt> <data_dir> <out.yaml>
// views.txt (tests/test_gpu_charuco_calibrate_host.py writes it from tests/charuco_calib_cases.py):
//   image_width image_height model n_dist dictionary
//   squares_x squares_y square_len marker_len first_id
//   n_views, then per view: n, then per corner: id x y
//   the calibrated fx fy cx cy k1 the caller expects (its own solve of the same views), and a tolerance in px / units of k1
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "camera_calibrator.hpp"
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

// the numbers of `data:` inside the block `key:` (one line, brackets stripped)
static std::vector<double> yamlData(const std::string &text, const std::string &key)
{
    std::vector<double> v;
    size_t at = text.find("\n" + key + ":");
    if (at == std::string::npos) return v;
    at = text.find("data:", at);
    if (at == std::string::npos) return v;
    const size_t from = text.find(':', at) + 1, to = text.find('\n', from);
    std::string s = text.substr(from, to - from);
    for (char &ch : s)
        if (ch == '[' || ch == ']' || ch == ',') ch = ' ';
    std::istringstream in(s);
    std::string tok;
    while (in >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));  // (strtod: round-trips %.17g)
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::printf("usage: %s <views.txt> <data dir> <out.yaml>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    int w = 0, h = 0, model = 0, n_dist = 0, dicno = 0, n_views = 0;
    fid_charuco_board board;
    std::memset(&board, 0, sizeof(board));
    in >> w >> h >> model >> n_dist >> dicno;
    in >> board.squares_x >> board.squares_y >> board.square_len >> board.marker_len >> board.first_id;
    in >> n_views;
    std::vector<std::vector<fid_charuco_corner>> views((size_t)(n_views > 0 ? n_views : 0));
    for (auto &v : views) {
        int n = 0;
        in >> n;
        v.resize((size_t)n);
        for (fid_charuco_corner &c : v) {
            std::memset(&c, 0, sizeof(c));
            in >> c.id >> c.x >> c.y;
        }
    }
    double expect[5], tol[2];
    for (double &e : expect) in >> e;
    in >> tol[0] >> tol[1];
    CHECK(bool(in) && n_views > 0);
    if (g_fail) return 1;

    Dictionary dict = getPredefinedDictionary(dicno, argv[2]);
    fid_dict fd = dict.view();
    fid_params params;
    fid_default_params(&params);
    fid_limits lim;
    fid_default_limits(&lim);
    lim.max_width = 640; lim.max_height = 480; lim.max_batch = 1;
    fid_ctx *ctx = nullptr;
    CHECK(fid_create(&params, &fd, &lim, 0, &ctx) == FID_OK);
    if (!ctx) return 1;

    CharucoCalibrator cal(ctx, w, h);
    CHECK(cal.size() == 0);
    for (const auto &v : views) cal.addView(v.data(), (int)v.size());
    cal.addView(nullptr, 0);  // a frame in which nothing was found: skipped, not an error
    CHECK(cal.size() == (size_t)n_views + 1);

    fid_calib_opts opts;
    fid_default_calib_opts(&opts);
    opts.free_mask = FID_CALIB_FREE_K | 1u << 4;
    opts.max_iter = 500;
    fid_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.model = model;
    cam.n_dist = n_dist;
    cam.K[0] = cam.K[4] = cam.K[8] = 1.;
    const fid_camera before = cam;
    fid_calib_out out;
    std::vector<fid_calib_view> vout;
    // without a board the call is refused and the camera stays
    CHECK(cal.calibrate(opts, &cam, &out, &vout) == FID_E_INVALID_ARG && std::memcmp(&cam, &before, sizeof(cam)) == 0);
    CHECK(std::strstr(fid_last_error(ctx), "board") != nullptr);
    CHECK(fid_set_charuco_board(ctx, &board) == FID_OK);
    const fid_status rc = cal.calibrate(opts, &cam, &out, &vout);
    CHECK(rc == FID_OK);
    if (rc != FID_OK) std::printf("fid_calibrate_charuco: %s\n", fid_last_error(ctx));
    CHECK(vout.size() == (size_t)n_views + 1 && out.n_views_used == n_views && vout.back().status == FID_CALIB_VIEW_FEW && vout.back().n_used == 0);
    CHECK(out.status == FID_CALIB_OK && out.cost <= out.start_cost && out.rms > 0. && out.rms < 2.);
    int n_points = 0;
    for (const auto &v : views) n_points += (int)v.size();
    CHECK(out.n_points == n_points && out.n_free == 5 + 6 * n_views);
    std::printf("rms %.6f px after %d trials; fx %.6f fy %.6f cx %.6f cy %.6f k1 %.8f\n", out.rms, out.n_iter, cam.K[0], cam.K[4], cam.K[2], cam.K[5], cam.D[0]);
    const double got[5] = {cam.K[0], cam.K[4], cam.K[2], cam.K[5], cam.D[0]};
    for (int i = 0; i < 5; i++) CHECK(std::fabs(got[i] - expect[i]) <= tol[i < 4 ? 0 : 1]);
    cal.clear();
    CHECK(cal.size() == 0);

    // ---- CameraInfo, the YAML file, and back
    CalibratedCameraInfo info;
    CHECK(CameraCalibrator::toCameraInfo(cam, w, h, &info));
    CHECK(info.distortion_model == "plumb_bob" && info.D.size() == 5 && info.width == (uint32_t)w && info.height == (uint32_t)h);
    CHECK(info.P[0] == cam.K[0] && info.P[2] == cam.K[2] && info.P[5] == cam.K[4] && info.P[6] == cam.K[5] && info.P[10] == 1.);
    CHECK(CameraCalibrator::writeYaml(argv[3], "calibrated", info));
    std::ifstream yf(argv[3]);
    std::stringstream ss;
    ss << yf.rdbuf();
    const std::string text = ss.str();
    const std::vector<double> Ky = yamlData(text, "camera_matrix"), Dy = yamlData(text, "distortion_coefficients");
    CHECK(Ky.size() == 9 && Dy.size() == 5 && yamlData(text, "projection_matrix").size() == 12);
    fid_camera back;
    CHECK(Ky.size() == 9 && fid_camera_from_info("plumb_bob", Ky.data(), Dy.data(), (int32_t)Dy.size(), &back) == FID_OK);
    CHECK(back.model == cam.model && back.n_dist == 5);
    CHECK(std::memcmp(back.K, cam.K, sizeof(cam.K)) == 0);
    for (int i = 0; i < 12; i++) CHECK(back.D[i] == (i < cam.n_dist ? cam.D[i] : 0.));

    fid_destroy(ctx);
    if (g_fail) {
        std::printf("%d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
