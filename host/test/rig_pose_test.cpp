// CameraRig (host/include/camera_rig.hpp): the frames of one time step -> fid_detect_batch -> the rig's pose in the map, the same from
// the markers handed back in, and what the caller recorded for the same frames.
//   usage: rig_pose_test <case.txt> <data dir> <frame0.pgm> <frame1.pgm> ...
// case.txt (tests/test_gpu_rig_pose_host.py writes it from tests/rig_cases.py; doubles printed to 17 digits: they read back bit for bit):
//   dictionary sigma_px
//   fx fy cx cy
//   n_cameras, then per camera x y z qx qy qz qw (the camera in the rig frame)
//   n_entries, then per map entry id len R (9) t (3)
//   what the caller found: n_markers start_camera rvec (3) tvec (3) image_error err_per_camera (n_cameras) cov_cam_pose (36)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "camera_rig.hpp"
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
    const size_t at = pix->size();
    pix->resize(at + (size_t)*w * *h);
    in.read((char *)pix->data() + at, (std::streamsize)((size_t)*w * *h));
    return bool(in);
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        std::printf("usage: %s <case.txt> <data dir> <frame0.pgm> [<frame1.pgm> ...]\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    int dicno = 0, n_cams = 0, n_entries = 0;
    double sigma_px = 0;
    CameraInfo info;
    info.distortion_model = "plumb_bob";
    info.D.assign(5, 0.);
    info.K[8] = 1.;
    in >> dicno >> sigma_px;
    in >> info.K[0] >> info.K[4] >> info.K[2] >> info.K[5];
    in >> n_cams;
    CameraRig rig("base_link");
    for (int c = 0; c < n_cams && in; c++) {
        double xyz[3], q[4];
        for (double &v : xyz) in >> v;
        for (double &v : q) in >> v;
        CHECK(rig.addCamera(info, xyz, q) == FID_OK);
    }
    in >> n_entries;
    std::vector<fid_map_entry> map((size_t)(n_entries > 0 ? n_entries : 0));
    for (fid_map_entry &e : map) {
        e.reserved0 = 0;
        in >> e.id >> e.len;
        for (double &v : e.R) in >> v;
        for (double &v : e.t) in >> v;
    }
    int want_n = 0, want_start = 0;
    double want_rvec[3], want_tvec[3], want_err = 0, want_cov[36];
    std::vector<double> want_per((size_t)(n_cams > 0 ? n_cams : 0));
    in >> want_n >> want_start;
    for (double &v : want_rvec) in >> v;
    for (double &v : want_tvec) in >> v;
    in >> want_err;
    for (double &v : want_per) in >> v;
    for (double &v : want_cov) in >> v;
    CHECK(bool(in) && n_cams >= 1 && argc - 3 == n_cams);
    if (g_fail) return 1;

    std::vector<uint8_t> pix;
    int W = 0, H = 0;
    for (int c = 0; c < n_cams; c++) {
        int w = 0, h = 0;
        CHECK(readPgm(argv[3 + c], &pix, &w, &h) && (c == 0 || (w == W && h == H)));
        W = w;
        H = h;
    }
    if (g_fail) return 1;

    Dictionary dict = getPredefinedDictionary(dicno, argv[2]);
    fid_dict fd = dict.view();
    fid_params params;
    fid_default_params(&params);
    fid_limits lim;
    fid_default_limits(&lim);
    lim.max_width = W; lim.max_height = H; lim.max_batch = n_cams;
    fid_ctx *ctx = nullptr;
    CHECK(fid_create(&params, &fd, &lim, 0, &ctx) == FID_OK);
    if (!ctx) return 1;
    {
        Header stamp;
        stamp.sec = 12;
        stamp.nsec = 34;
        std::vector<RigPose> poses;
        // nothing is set yet: the refusals say what is missing
        const int cap = 64;
        std::vector<fid_marker> markers((size_t)n_cams * cap);
        std::vector<int32_t> n((size_t)n_cams, 0);
        CHECK(fid_detect_batch(ctx, pix.data(), n_cams, W, H, W, (int64_t)W * H, FID_ENC_MONO8, markers.data(), cap, n.data()) == FID_OK);
        CHECK(rig.pose(ctx, stamp, &poses) == FID_E_INVALID_ARG && rig.lastError().find("no rig") != std::string::npos);
        CHECK(rig.apply(ctx) == FID_OK);
        CHECK(rig.pose(ctx, stamp, &poses) == FID_E_INVALID_ARG && rig.lastError().find("no map") != std::string::npos);
        CHECK(fid_set_map(ctx, map.data(), (int32_t)map.size()) == FID_OK);
        int32_t steps = -1;
        CHECK(fid_rig_steps_last(ctx, &steps) == FID_OK && steps == 1);

        // the time step of the last call, with its covariance
        CHECK(rig.pose(ctx, stamp, &poses, sigma_px) == FID_OK && poses.size() == 1);
        if (poses.size() == 1) {
            const RigPose &p = poses[0];
            std::printf("%d markers over %d cameras, start camera %d, rig at %.4f %.4f %.4f\n", p.record.n_markers, p.record.n_cameras, p.record.start_camera,
                        p.pose.pose.px, p.pose.pose.py, p.pose.pose.pz);
            CHECK(p.valid && p.record.n_markers == want_n && p.record.start_camera == want_start && p.record.reserved0 == 0);
            for (int a = 0; a < 3; a++) CHECK(p.record.rvec[a] == want_rvec[a] && p.record.tvec[a] == want_tvec[a]);
            CHECK(p.record.image_error == want_err && (int)p.err_per_camera.size() == n_cams);
            for (int c = 0; c < n_cams && c < (int)p.err_per_camera.size(); c++) CHECK(p.err_per_camera[(size_t)c] == want_per[(size_t)c]);
            for (int i = 0; i < 36; i++) CHECK(p.pose.covariance[(size_t)i] == want_cov[i]);
            CHECK(p.pose.header.frame_id == "map" && p.child_frame_id == "base_link" && p.pose.header.sec == 12 && p.pose.header.nsec == 34);
            CHECK(p.pose.pose.px == p.record.rig_t[0] && p.pose.pose.py == p.record.rig_t[1] && p.pose.pose.pz == p.record.rig_t[2]);
            const double qn = p.pose.pose.ox * p.pose.pose.ox + p.pose.pose.oy * p.pose.pose.oy + p.pose.pose.oz * p.pose.pose.oz + p.pose.pose.ow * p.pose.pose.ow;
            CHECK(std::fabs(qn - 1.) < 1e-12);
            // the quaternion is rig_R: its first column
            const double x = p.pose.pose.ox, y = p.pose.pose.oy, z = p.pose.pose.oz, w = p.pose.pose.ow;
            CHECK(std::fabs(1 - 2 * (y * y + z * z) - p.record.rig_R[0]) < 1e-12 && std::fabs(2 * (x * y + z * w) - p.record.rig_R[3]) < 1e-12 &&
                  std::fabs(2 * (x * z - y * w) - p.record.rig_R[6]) < 1e-12);

            // the same from the markers handed back in, and without the covariance: the same pose bytes
            std::vector<fid_marker> flat;
            for (int c = 0; c < n_cams; c++) flat.insert(flat.end(), markers.begin() + (long)c * cap, markers.begin() + (long)c * cap + n[(size_t)c]);
            fid_rig_pose_out again;
            CHECK(fid_rig_pose(ctx, flat.data(), n.data(), &again, 0., nullptr) == FID_OK && std::memcmp(&again, &p.record, sizeof(again)) == 0);
            std::vector<RigPose> plain;
            CHECK(rig.pose(ctx, stamp, &plain) == FID_OK && plain.size() == 1 && std::memcmp(&plain[0].record, &p.record, sizeof(again)) == 0);
            bool zero = true;
            for (double v : plain[0].pose.covariance) zero = zero && v == 0.;
            CHECK(zero);
        }
        // a rig of one camera more than the frames of the call: no whole number of time steps
        if (n_cams == 2) {
            CameraRig three = rig;
            const double xyz[3] = {0., 0.1, 0.}, q[4] = {0., 0., 0., 1.};
            CHECK(three.addCamera(info, xyz, q) == FID_OK && three.apply(ctx) == FID_OK);
            CHECK(three.pose(ctx, stamp, &poses) == FID_E_INVALID_ARG && three.lastError().find("multiple") != std::string::npos);
            CHECK(rig.apply(ctx) == FID_OK);
        }
        CameraInfo odd = info;
        odd.distortion_model = "unified";
        const double xyz0[3] = {0., 0., 0.}, q0[4] = {0., 0., 0., 0.};
        CameraRig bad;
        CHECK(bad.addCamera(odd, xyz0, q0) == FID_E_UNSUPPORTED && bad.addCamera(info, xyz0, q0) == FID_E_INVALID_ARG && bad.size() == 0);
    }
    fid_destroy(ctx);
    if (g_fail) return 1;
    std::printf("all checks passed\n");
    return 0;
}
