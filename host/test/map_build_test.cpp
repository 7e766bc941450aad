// MapBuilder (host/include/map_builder.hpp): views -> build -> save -> fid_map_load_file -> fid_set_map -> fid_map_pose_cam on one of
// the views gives that view's pose.
//   usage: map_build_test <views.txt> <data_dir> <out map file>
// views.txt (tests/test_gpu_map_build_host.py writes it from tests/map_build_cases.py):
//   fx fy cx cy k1 k2 p1 p2 k3 fiducial_len dictionary
//   the fixed entry: id len, R (9, row-major), t (3)
//   n_views, then per view: n, then per marker: id c0 .. c7
//   n_expected, then per marker the caller expects solved: id x y z, and a tolerance in metres (its own solve of the same views)
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

// cv::Rodrigues, vector -> matrix (row-major)
static void rotationMatrix(const double r[3], double R[9])
{
    const double th = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1. : 0.;
    if (th < 1e-300) return;
    const double k[3] = {r[0] / th, r[1] / th, r[2] / th}, s = std::sin(th), c = std::cos(th);
    const double kx[9] = {0., -k[2], k[1], k[2], 0., -k[0], -k[1], k[0], 0.};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = c * (i == j ? 1. : 0.) + (1. - c) * k[i] * k[j] + s * kx[3 * i + j];
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::printf("usage: %s <views.txt> <data dir> <out map file>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    fid_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.model = FID_CAM_PLUMB_BOB;
    cam.n_dist = 5;
    cam.K[8] = 1.;
    double len = 0;
    int dicno = 0, n_views = 0, n_expected = 0;
    in >> cam.K[0] >> cam.K[4] >> cam.K[2] >> cam.K[5];
    for (int i = 0; i < 5; i++) in >> cam.D[i];
    in >> len >> dicno;
    std::vector<fid_map_entry> fixed(1);
    std::memset(&fixed[0], 0, sizeof(fid_map_entry));
    in >> fixed[0].id >> fixed[0].len;
    for (double &r : fixed[0].R) in >> r;
    for (double &t : fixed[0].t) in >> t;
    in >> n_views;
    std::vector<std::vector<fid_marker>> views((size_t)(n_views > 0 ? n_views : 0));
    for (auto &v : views) {
        int n = 0;
        in >> n;
        v.resize((size_t)n);
        for (fid_marker &m : v) {
            in >> m.id;
            for (float &c : m.corners) in >> c;
        }
    }
    in >> n_expected;
    std::vector<int> eid((size_t)(n_expected > 0 ? n_expected : 0));
    std::vector<double> ex(3 * eid.size()), etol(eid.size());
    for (size_t k = 0; k < eid.size(); k++) in >> eid[k] >> ex[3 * k] >> ex[3 * k + 1] >> ex[3 * k + 2] >> etol[k];
    CHECK(bool(in) && n_views > 0 && n_expected > 0);
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
    CHECK(mb.size() == 0);
    for (const auto &v : views) mb.addView(v.data(), (int)v.size());
    mb.addView(nullptr, 0);  // a frame in which nothing was found: reported, not an error
    CHECK(mb.size() == (size_t)n_views + 1);

    fid_build_opts opts;
    fid_default_build_opts(&opts);
    opts.fiducial_len = len;
    opts.max_iter = 500;
    opts.eps = 1e-15;
    fid_build_out out;
    std::vector<fid_build_marker> markers;
    std::vector<fid_map_entry> entries;
    std::vector<fid_build_view> vout;
    const fid_status rc = mb.build(cam, fixed, opts, &out, &markers, &entries, &vout);
    CHECK(rc == FID_OK);
    if (rc != FID_OK) {
        std::printf("fid_build_map_cam: %s\n", fid_last_error(ctx));
        return 1;
    }
    CHECK(vout.size() == (size_t)n_views + 1 && out.n_views_used == n_views && vout.back().status == FID_BUILD_VIEW_FEW);
    CHECK(out.n_fixed == 1 && (size_t)out.n_markers == entries.size() && out.cost <= out.start_cost);
    std::printf("status %d trials %d markers %d rms %.4f px\n", out.status, out.n_iter, out.n_markers, out.rms);
    for (size_t k = 0; k < eid.size(); k++) {
        bool found = false;
        for (const fid_build_marker &m : markers) {
            if (m.id != eid[k]) continue;
            found = true;
            CHECK(m.status == FID_BUILD_MARKER_SOLVED);
            for (int a = 0; a < 3; a++) CHECK(std::fabs(m.entry.t[a] - ex[3 * k + a]) <= etol[k]);
            CHECK(m.cov[21] > 0. && m.cov[28] > 0. && m.cov[35] > 0.);
        }
        CHECK(found);
    }

    // the file, read back to the printed decimals
    CHECK(MapBuilder::save(argv[3], markers) == FID_OK);
    std::vector<fid_map_entry> loaded(entries.size() + 1);
    int32_t n_loaded = 0, n_skipped = 0;
    CHECK(fid_map_load_file(argv[3], len, loaded.data(), (int32_t)loaded.size(), &n_loaded, &n_skipped) == FID_OK);
    CHECK((size_t)n_loaded == entries.size() && n_skipped == 0);
    for (int k = 0; k < n_loaded && (size_t)k < entries.size(); k++) {
        CHECK(loaded[k].id == entries[k].id);
        for (int a = 0; a < 3; a++) CHECK(std::fabs(loaded[k].t[a] - entries[k].t[a]) <= 1e-6);
        for (int a = 0; a < 9; a++) CHECK(std::fabs(loaded[k].R[a] - entries[k].R[a]) <= 1e-7);
    }

    // the built map poses the camera of its own views where the solve left them (to what the file's decimals allow)
    CHECK(fid_set_map(ctx, loaded.data(), n_loaded) == FID_OK);
    for (int v = 0; v < n_views; v += (n_views > 3 ? n_views / 3 : 1)) {
        fid_map_pose_out p;
        CHECK(fid_map_pose_cam(ctx, &cam, views[(size_t)v].data(), (int32_t)views[(size_t)v].size(), &p) == FID_OK);
        CHECK(p.n_markers == vout[(size_t)v].n_used);
        double d = 0, R[9];  // (as matrices: near a half turn a rotation has two vectors)
        rotationMatrix(vout[(size_t)v].rvec, R);
        for (int a = 0; a < 9; a++) d = std::fmax(d, std::fabs(p.R[a] - R[a]));
        for (int a = 0; a < 3; a++) d = std::fmax(d, std::fabs(p.tvec[a] - vout[(size_t)v].tvec[a]));
        std::printf("view %d: fid_map_pose_cam against the built map differs from the solve's pose by %.2e\n", v, d);
        CHECK(d <= 1e-4);  // (the file keeps micrometres and microdegrees; the pose is a least-squares fit of the same corners)
    }
    fid_destroy(ctx);
    if (g_fail) return 1;
    std::printf("all checks passed\n");
    return 0;
}
