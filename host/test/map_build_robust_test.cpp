// MapBuilder::buildRobust (host/include/map_builder.hpp): views with planted wrong observations -> the trimmed build names them, and
// what the class returns is what fid_build_map_robust_cam returns on the same views, byte for byte.
//   usage: map_build_robust_test <views.txt> <data_dir>
// views.txt (tests/test_gpu_map_build_robust_host.py writes it from tests/map_build_robust_cases.py):
//   fx fy cx cy k1 k2 p1 p2 k3 fiducial_len dictionary inlier_px min_views_place min_views
//   the fixed entry: id len, R (9, row-major), t (3)
//   n_views, then per view: n, then per marker: id c0 .. c7 state     (state: the FID_BUILD_OBS_* the caller expects)
//   rounds stable
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "fiducials_host.hpp"
#include "map_builder.hpp"

using namespace fiducials_amd;

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::printf("usage: %s <views.txt> <data dir>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    fid_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.model = FID_CAM_PLUMB_BOB;
    cam.n_dist = 5;
    cam.K[8] = 1.;
    double len = 0;
    int dicno = 0, n_views = 0, min_views = 2, rounds = 0, stable = 0;
    fid_build_robust_opts ropts;
    std::memset(&ropts, 0, sizeof(ropts));
    in >> cam.K[0] >> cam.K[4] >> cam.K[2] >> cam.K[5];
    for (int i = 0; i < 5; i++) in >> cam.D[i];
    in >> len >> dicno >> ropts.inlier_px >> ropts.min_views_place >> min_views;
    std::vector<fid_map_entry> fixed(1);
    std::memset(&fixed[0], 0, sizeof(fid_map_entry));
    in >> fixed[0].id >> fixed[0].len;
    for (double &r : fixed[0].R) in >> r;
    for (double &t : fixed[0].t) in >> t;
    in >> n_views;
    std::vector<std::vector<fid_marker>> views((size_t)(n_views > 0 ? n_views : 0));
    std::vector<std::vector<int>> expect(views.size());
    size_t cap = 1, total = 0;
    for (size_t v = 0; v < views.size(); v++) {
        int n = 0;
        in >> n;
        views[v].resize((size_t)n);
        expect[v].resize((size_t)n);
        for (size_t k = 0; k < views[v].size(); k++) {
            in >> views[v][k].id;
            for (float &c : views[v][k].corners) in >> c;
            in >> expect[v][k];
        }
        cap = views[v].size() > cap ? views[v].size() : cap;
        total += views[v].size();
    }
    in >> rounds >> stable;
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

    MapBuilder mb(ctx);
    for (const auto &v : views) mb.addView(v.data(), (int)v.size());
    fid_build_opts opts;
    fid_default_build_opts(&opts);
    opts.fiducial_len = len;
    opts.min_views = min_views;
    opts.max_iter = 500;
    opts.eps = 1e-15;
    fid_build_out out;
    MapBuilder::RobustReport rep;
    std::vector<fid_build_marker> markers;
    std::vector<fid_map_entry> entries;
    std::vector<fid_build_view> vout;
    const fid_status rc = mb.buildRobust(cam, fixed, opts, ropts, &out, &rep, &markers, &entries, &vout);
    CHECK(rc == FID_OK);
    if (rc != FID_OK) {
        std::printf("fid_build_map_robust_cam: %s\n", fid_last_error(ctx));
        return 1;
    }
    std::printf("rounds %d stable %d inliers %d outliers %d worst inlier %.3f px best outlier %.3f px rms %.4f px\n", rep.out.rounds, rep.out.stable, rep.out.n_inliers,
                rep.out.n_outliers, rep.out.worst_inlier_px, rep.out.best_outlier_px, out.rms);
    CHECK(rep.out.rounds == rounds && rep.out.stable == stable);
    int n_out = 0;
    for (size_t v = 0; v < views.size(); v++) {
        CHECK(rep.obs_state[v].size() == views[v].size() && rep.obs_err_px[v].size() == views[v].size());
        int here = 0;
        for (size_t k = 0; k < views[v].size(); k++) {
            CHECK((int)rep.obs_state[v][k] == expect[v][k]);
            if (rep.obs_state[v][k] == FID_BUILD_OBS_OUTLIER) here++;
            if (rep.obs_state[v][k] == FID_BUILD_OBS_INLIER) CHECK(rep.obs_err_px[v][k] >= 0. && rep.obs_err_px[v][k] <= ropts.inlier_px);
        }
        CHECK(rep.view_outliers[v] == here);
        n_out += here;
    }
    CHECK(n_out == rep.out.n_outliers && rep.marker_outliers.size() == markers.size());

    // the C call on the same views: the same bytes
    std::vector<fid_marker> packed(views.size() * cap);
    std::vector<int32_t> n(views.size());
    for (size_t v = 0; v < views.size(); v++) {
        n[v] = (int32_t)views[v].size();
        for (size_t k = 0; k < views[v].size(); k++) packed[v * cap + k] = views[v][k];
    }
    std::vector<fid_build_marker> mout(total);
    std::vector<fid_build_view> vo2(views.size());
    std::vector<uint8_t> state(views.size() * cap);
    std::vector<double> err(views.size() * cap);
    std::vector<int32_t> mo(total), vo(views.size());
    fid_build_out out2;
    fid_build_robust_out rout2;
    int32_t nm = 0;
    CHECK(fid_build_map_robust_cam(ctx, &cam, packed.data(), n.data(), (int32_t)views.size(), (int32_t)cap, fixed.data(), 1, &opts, &ropts, &out2, &rout2, mout.data(),
                                   (int32_t)mout.size(), &nm, vo2.data(), state.data(), err.data(), mo.data(), vo.data()) == FID_OK);
    CHECK(std::memcmp(&out, &out2, sizeof(out)) == 0 && std::memcmp(&rep.out, &rout2, sizeof(rout2)) == 0);
    CHECK((size_t)nm == markers.size() && std::memcmp(markers.data(), mout.data(), sizeof(fid_build_marker) * markers.size()) == 0);
    CHECK(std::memcmp(vout.data(), vo2.data(), sizeof(fid_build_view) * vout.size()) == 0);
    CHECK(std::memcmp(rep.view_outliers.data(), vo.data(), sizeof(int32_t) * vo.size()) == 0);
    CHECK(std::memcmp(rep.marker_outliers.data(), mo.data(), sizeof(int32_t) * markers.size()) == 0);
    for (size_t v = 0; v < views.size(); v++) {
        CHECK(views[v].empty() || std::memcmp(rep.obs_state[v].data(), &state[v * cap], views[v].size()) == 0);
        CHECK(views[v].empty() || std::memcmp(rep.obs_err_px[v].data(), &err[v * cap], sizeof(double) * views[v].size()) == 0);
    }
    fid_destroy(ctx);
    if (g_fail) return 1;
    std::printf("all checks passed\n");
    return 0;
}
