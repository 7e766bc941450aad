// aruco_map_robust_test.cpp -- FiducialsNode (host/include/fiducials_host.hpp) with ~map_outlier_px: the consensus map pose.
//   usage: aruco_map_robust_test <frame.pgm> <lying_map.txt> <all_wrong_map.txt> <camera.txt> <data_dir> <dictionary> <fiducial_len>
//   camera.txt: "fx fy cx cy", then "inlier_px", then the two ids whose map entries lie.
// checks that with ~map_outlier_px = 0 the serialised outputs and the map pose are those of a node that never heard of the
// parameter; that with it on and the lying map PoseOutputs::map_outliers names the two ids and map_pose equals
// fid_map_pose_robust_last_cam's cam_t / cam_R for the same frame on a context of its own (twice: the second frame rides in the
// detect call); that ~pose_covariance then reports fid_map_pose_cov_cam's covariance over the inliers; and that a map in which
// every entry is wrong gives an empty map_pose and every used id as an outlier.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

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

static bool samePose(const PoseStamped &a, const PoseStamped &b)
{
    return a.header.frame_id == b.header.frame_id && a.pose.px == b.pose.px && a.pose.py == b.pose.py && a.pose.pz == b.pose.pz && a.pose.ox == b.pose.ox &&
           a.pose.oy == b.pose.oy && a.pose.oz == b.pose.oz && a.pose.ow == b.pose.ow;
}

int main(int argc, char **argv)
{
    if (argc < 8) {
        std::printf("usage: %s <frame.pgm> <lying_map.txt> <all_wrong_map.txt> <camera.txt> <data dir> <dictionary> <fiducial_len>\n", argv[0]);
        return 2;
    }
    try {
        std::ifstream f(argv[1], std::ios::binary);
        std::string magic;
        int w, h, maxv;
        f >> magic >> w >> h >> maxv;
        f.get();
        Image img;
        img.width = w; img.height = h; img.step = w; img.encoding = "mono8";
        img.header.seq = 9; img.header.sec = 55; img.header.nsec = 3; img.header.frame_id = "camera";
        img.data.resize((size_t)w * h);
        f.read((char *)img.data.data(), (std::streamsize)img.data.size());
        CameraInfo cam;
        cam.header.frame_id = "camera";
        double inlier_px = 0;
        int lie[2] = {-1, -1};
        {
            std::ifstream e(argv[4]);
            double fx, fy, cx, cy;
            e >> fx >> fy >> cx >> cy >> inlier_px >> lie[0] >> lie[1];
            cam.K = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
            cam.D = {0.05, -0.02, 0.001, -0.0005, 0};
        }
        FiducialsNode::Params p;
        p.data_dir = argv[5];
        p.dictionary = std::atoi(argv[6]);
        p.fiducial_len = std::atof(argv[7]);
        p.max_width = w;
        p.max_height = h;
        p.map_file = argv[2];
        // ---- off: a node that never heard of the parameter, and one with map_outlier_px = 0 (map_min_markers is then not read)
        FiducialArray fa0, fa1;
        PoseOutputs o0, o1;
        {
            FiducialsNode never(p);
            never.camInfoCallback(cam);
            CHECK(never.imageCallback(img, &fa0) && never.poseEstimateCallback(fa0, &o0));
            FiducialsNode::Params poff = p;
            poff.map_outlier_px = 0.0;
            poff.map_min_markers = 5;
            FiducialsNode off(poff);
            off.camInfoCallback(cam);
            CHECK(off.imageCallback(img, &fa1) && off.poseEstimateCallback(fa1, &o1));
            CHECK(serialize(fa0) == serialize(fa1) && serialize(o0.fta) == serialize(o1.fta) && o0.tf.size() == o1.tf.size());
            CHECK(o0.map_pose.size() == 1 && o1.map_pose.size() == 1 && o0.map_outliers.empty() && o1.map_outliers.empty());
            if (o0.map_pose.size() == 1 && o1.map_pose.size() == 1) CHECK(samePose(o0.map_pose[0], o1.map_pose[0]));
        }
        // ---- the same frame through the C interface on a context of its own
        std::vector<fid_map_entry> entries(FID_MAP_MAX_ENTRIES);
        int32_t n_entries = 0, skipped = 0;
        CHECK(fid_map_load_file(argv[2], p.fiducial_len, entries.data(), (int32_t)entries.size(), &n_entries, &skipped) == FID_OK);
        Dictionary dict = getPredefinedDictionary(p.dictionary, p.data_dir);
        fid_dict fd = dict.view();
        fid_limits lim;
        fid_default_limits(&lim);
        lim.max_width = w; lim.max_height = h; lim.max_batch = 1;
        fid_ctx *ctx = nullptr;
        CHECK(fid_create(&p.detector, &fd, &lim, 0, &ctx) == FID_OK);
        std::vector<fid_marker> mk(1024);
        int32_t n = 0;
        fid_camera fc;
        CHECK(fid_camera_from_info("plumb_bob", cam.K.data(), cam.D.data(), 5, &fc) == FID_OK);
        const fid_map_robust_opts opts = {inlier_px, 2, 0};
        fid_map_pose_out want;
        fid_map_robust_out rob;
        CHECK(fid_set_map(ctx, entries.data(), n_entries) == FID_OK);
        CHECK(fid_detect(ctx, img.data.data(), w, h, w, FID_ENC_MONO8, mk.data(), (int32_t)mk.size(), &n) == FID_OK);
        CHECK(fid_map_pose_robust_last_cam(ctx, &fc, &opts, &want, &rob, 1) == FID_OK);
        CHECK(rob.status == FID_MAP_ROBUST_OK && rob.n_outliers == 2 && want.n_markers == rob.n_used - 2);
        // ---- on, with the lying map
        FiducialsNode::Params pon = p;
        pon.map_outlier_px = inlier_px;
        pon.pose_covariance = true;
        pon.pose_covariance_sigma_px = 0.5;
        {
            FiducialsNode node(pon);
            node.camInfoCallback(cam);
            FiducialArray fa;
            PoseOutputs out;
            for (int round = 0; round < 2; round++) {
                CHECK(node.imageCallback(img, &fa) && node.poseEstimateCallback(fa, &out));
                CHECK(serialize(fa) == serialize(fa0) && serialize(out.fta) == serialize(o0.fta));
                std::vector<int32_t> got = out.map_outliers;
                std::sort(got.begin(), got.end());
                CHECK(got.size() == 2 && got[0] == std::min(lie[0], lie[1]) && got[1] == std::max(lie[0], lie[1]));
                CHECK(out.map_pose.size() == 1 && out.map_pose_cov.size() == 1);
                if (out.map_pose.size() != 1 || out.map_pose_cov.size() != 1) continue;
                const PoseStamped &ps = out.map_pose[0];
                CHECK(ps.header.frame_id == "map" && ps.header.sec == 55 && ps.header.nsec == 3);
                CHECK(ps.pose.px == want.cam_t[0] && ps.pose.py == want.cam_t[1] && ps.pose.pz == want.cam_t[2]);
                const double x = ps.pose.ox, y = ps.pose.oy, z = ps.pose.oz, qw = ps.pose.ow;
                const double Rq[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * qw), 2 * (x * z + y * qw), 2 * (x * y + z * qw), 1 - 2 * (x * x + z * z),
                                      2 * (y * z - x * qw), 2 * (x * z - y * qw), 2 * (y * z + x * qw), 1 - 2 * (x * x + y * y)};
                for (int i = 0; i < 9; i++) CHECK(std::fabs(Rq[i] - want.cam_R[i]) < 1e-12);
                CHECK(!samePose(ps, o0.map_pose.empty() ? ps : o0.map_pose[0]));  // (the plain pose of the lying map is another)
                // the covariance: fid_map_pose_cov_cam over the inliers
                std::vector<fid_marker> inl;
                for (int i = 0; i < n; i++)
                    if (mk[(size_t)i].id != lie[0] && mk[(size_t)i].id != lie[1]) inl.push_back(mk[(size_t)i]);
                fid_map_pose_out again;
                fid_map_pose_cov cov;
                CHECK(fid_map_pose_cov_cam(ctx, &fc, inl.data(), (int32_t)inl.size(), &again, 0.5, &cov) == FID_OK && cov.pose.status == 0);
                CHECK(std::memcmp(&again, &want, sizeof again) == 0);
                CHECK(out.map_pose_cov[0].pose.px == ps.pose.px && out.map_pose_cov[0].pose.ow == ps.pose.ow);
                bool same = true, any = false;
                for (int i = 0; i < 36; i++) {
                    same = same && out.map_pose_cov[0].covariance[(size_t)i] == cov.cov_cam_pose[i];
                    any = any || cov.cov_cam_pose[i] != 0.;
                }
                CHECK(same && any);
            }
        }
        // ---- every entry wrong: no consensus, no pose, every used id an outlier
        {
            FiducialsNode::Params pw = pon;
            pw.map_file = argv[3];
            FiducialsNode node(pw);
            node.camInfoCallback(cam);
            FiducialArray fa;
            PoseOutputs out;
            CHECK(node.imageCallback(img, &fa) && node.poseEstimateCallback(fa, &out));
            CHECK(out.map_pose.empty() && out.map_pose_cov.empty() && (int)out.map_outliers.size() == rob.n_used);
            CHECK(serialize(out.fta) == serialize(o0.fta));
        }
        fid_destroy(ctx);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    std::printf(g_fail ? "%d check(s) failed\n" : "all checks passed%.0d\n", g_fail);
    return g_fail ? 1 : 0;
}
