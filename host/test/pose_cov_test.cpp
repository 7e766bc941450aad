// pose_cov_test.cpp -- FiducialsNode and StagNode with ~pose_covariance (host/include/fiducials_host.hpp, stag_host.hpp).
//   usage: pose_cov_test <frame.pgm> <map.txt> <camera.txt> <data_dir> <dictionary> <fiducial_len> <stag_frame.pgm> <stag HD>
//   camera.txt: "fx fy cx cy".  frame.pgm: a scene of the map's fiducials; stag_frame.pgm: STag markers of library <stag HD>.
// checks that with pose_covariance off the node's outputs are the default node's (the serialised messages byte for byte); that with
// it on and vis_msgs every hypothesis carries fid_pose_last_cov_cam's cov_pose for the same frame and camera (equal, not close), the
// poses being what they were; that with a map file map_pose_cov has one entry with fid_map_pose_last_cov_cam's cov_cam_pose and
// map_pose is unchanged; and the same for StagNode's Detection2DArray against fid_stag_pose_last_cov_cam.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

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

static Image readPgm(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    std::string magic;
    int w = 0, h = 0, maxv = 0;
    f >> magic >> w >> h >> maxv;
    f.get();
    Image img;
    img.width = w; img.height = h; img.step = w; img.encoding = "mono8";
    img.header.seq = 4; img.header.sec = 21; img.header.nsec = 8; img.header.frame_id = "camera";
    img.data.resize((size_t)w * h);
    f.read((char *)img.data.data(), (std::streamsize)img.data.size());
    return img;
}

static bool samePose(const Pose &a, const Pose &b)
{
    return a.px == b.px && a.py == b.py && a.pz == b.pz && a.ox == b.ox && a.oy == b.oy && a.oz == b.oz && a.ow == b.ow;
}
static bool allZero(const std::array<double, 36> &c)
{
    for (double v : c)
        if (v != 0.) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 9) {
        std::printf("usage: %s <frame.pgm> <map.txt> <camera.txt> <data dir> <dictionary> <fiducial_len> <stag_frame.pgm> <stag HD>\n", argv[0]);
        return 2;
    }
    try {
        const Image img = readPgm(argv[1]);
        const int w = (int)img.width, h = (int)img.height;
        CameraInfo cam;
        cam.header.frame_id = "camera";
        cam.distortion_model = "plumb_bob";
        cam.D = {0.05, -0.02, 0.001, -0.0005, 0.0};
        {
            std::ifstream e(argv[3]);
            double fx, fy, cx, cy;
            e >> fx >> fy >> cx >> cy;
            cam.K = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
        }
        FiducialsNode::Params p;
        p.data_dir = argv[4];
        p.dictionary = std::atoi(argv[5]);
        p.fiducial_len = std::atof(argv[6]);
        p.max_width = w;
        p.max_height = h;
        auto run = [&](const FiducialsNode::Params &pp, FiducialArray *fa, PoseOutputs *out) {
            FiducialsNode node(pp);
            node.camInfoCallback(cam);
            bool posed = false;
            for (int frame = 0; frame < 2; frame++) {  // (the second frame's poses come out of the detect call's stream)
                CHECK(node.imageCallback(img, fa));
                *out = PoseOutputs();
                posed = node.poseEstimateCallback(*fa, out);
            }
            return posed;
        };
        FiducialArray fa0, fa;
        PoseOutputs o0, o;
        // ---- off is the default node: the fiducial_msgs view byte for byte, the vision_msgs view with zero covariances
        CHECK(run(p, &fa0, &o0));
        CHECK(fa0.fiducials.size() >= 3 && o0.fta.transforms.size() == fa0.fiducials.size() && o0.map_pose_cov.empty());
        FiducialsNode::Params poff = p;
        poff.pose_covariance = false;
        poff.pose_covariance_sigma_px = 3.0;  // (not read while off)
        CHECK(run(poff, &fa, &o));
        CHECK(serialize(fa) == serialize(fa0) && serialize(o.fta) == serialize(o0.fta) && o.tf.size() == o0.tf.size() && o.map_pose_cov.empty());
        FiducialsNode::Params pon = p;
        pon.pose_covariance = true;
        CHECK(run(pon, &fa, &o));
        CHECK(serialize(fa) == serialize(fa0) && serialize(o.fta) == serialize(o0.fta));  // (fiducial_msgs has no slot: unchanged)
        // ---- on, vis_msgs, with the map: the library's own records on a context of its own
        PoseOutputs v0, v;
        FiducialsNode::Params pv = p;
        pv.vis_msgs = true;
        pv.map_file = argv[2];
        CHECK(run(pv, &fa, &v0));
        CHECK(v0.vma.detections.size() == fa0.fiducials.size() && v0.map_pose.size() == 1 && v0.map_pose_cov.empty());
        for (const Detection2D &d : v0.vma.detections) CHECK(d.results.size() == 1 && allZero(d.results[0].covariance));
        pv.pose_covariance = true;
        pv.pose_covariance_sigma_px = 0.5;
        CHECK(run(pv, &fa, &v));
        CHECK(v.vma.detections.size() == v0.vma.detections.size() && v.map_pose.size() == 1 && v.map_pose_cov.size() == 1);
        Dictionary dict = getPredefinedDictionary(p.dictionary, p.data_dir);
        fid_dict fd = dict.view();
        fid_limits lim;
        fid_default_limits(&lim);
        lim.max_width = w; lim.max_height = h; lim.max_batch = 1;
        fid_ctx *ctx = nullptr;
        CHECK(fid_create(&p.detector, &fd, &lim, 0, &ctx) == FID_OK);
        fid_camera camera;
        CHECK(fid_camera_from_info("plumb_bob", cam.K.data(), cam.D.data(), 5, &camera) == FID_OK);
        std::vector<fid_marker> mk((size_t)lim.max_markers_per_frame);
        int32_t n = 0;
        CHECK(fid_detect(ctx, img.data.data(), w, h, w, FID_ENC_MONO8, mk.data(), (int32_t)mk.size(), &n) == FID_OK && n == (int32_t)fa0.fiducials.size());
        std::vector<fid_pose_out> poses((size_t)lim.max_markers_per_frame);
        std::vector<fid_pose_cov> covs((size_t)lim.max_markers_per_frame);
        CHECK(fid_pose_last_cov_cam(ctx, &camera, p.fiducial_len, poses.data(), (int32_t)poses.size(), 0.5, covs.data()) == FID_OK);
        for (size_t i = 0; i < v.vma.detections.size() && i < (size_t)n; i++) {
            const ObjectHypothesisWithPose &hyp = v.vma.detections[i].results[0], &hyp0 = v0.vma.detections[i].results[0];
            CHECK(hyp.id == mk[i].id && hyp.id == hyp0.id && hyp.score == hyp0.score && samePose(hyp.pose, hyp0.pose));
            CHECK(covs[i].status == 0 && !allZero(hyp.covariance));
            CHECK(std::memcmp(hyp.covariance.data(), covs[i].cov_pose, sizeof(double) * 36) == 0);
            CHECK(hyp.pose.px == poses[i].tvec[0] && hyp.pose.pz == poses[i].tvec[2]);
        }
        // the map
        std::vector<fid_map_entry> entries(FID_MAP_MAX_ENTRIES);
        int32_t n_entries = 0, skipped = 0;
        CHECK(fid_map_load_file(argv[2], p.fiducial_len, entries.data(), (int32_t)entries.size(), &n_entries, &skipped) == FID_OK && n_entries > 0);
        CHECK(fid_set_map(ctx, entries.data(), n_entries) == FID_OK);
        fid_map_pose_out mp;
        fid_map_pose_cov mcov;
        CHECK(fid_map_pose_last_cov_cam(ctx, &camera, &mp, 1, 0.5, &mcov) == FID_OK && mp.n_markers > 0 && mcov.pose.status == 0);
        if (v.map_pose_cov.size() == 1 && v.map_pose.size() == 1 && v0.map_pose.size() == 1) {
            CHECK(samePose(v.map_pose[0].pose, v0.map_pose[0].pose) && v.map_pose[0].header.frame_id == "map");
            CHECK(samePose(v.map_pose_cov[0].pose, v.map_pose[0].pose) && v.map_pose_cov[0].header.frame_id == "map");
            CHECK(std::memcmp(v.map_pose_cov[0].covariance.data(), mcov.cov_cam_pose, sizeof(double) * 36) == 0 && !allZero(v.map_pose_cov[0].covariance));
            CHECK(v.map_pose[0].pose.px == mp.cam_t[0]);
        }
        fid_destroy(ctx);
        // ---- StagNode: the Detection2DArray's hypotheses against fid_stag_pose_last_cov_cam
        {
            const Image simg = readPgm(argv[7]);
            StagNode::Params sp;
            sp.libraryHD = std::atoi(argv[8]);
            StagNode::Outputs s0, s1;
            {
                StagNode node(sp, argv[4], (int)simg.width, (int)simg.height);
                node.cameraInfoCallback(cam);
                CHECK(node.imageCallback(simg, &s0) && s0.array_published && s0.array.detections.size() >= 2);
            }
            for (const Detection2D &d : s0.array.detections) CHECK(d.results.size() == 1 && allZero(d.results[0].covariance));
            sp.pose_covariance = true;
            sp.pose_covariance_sigma_px = 0.5;
            {
                StagNode node(sp, argv[4], (int)simg.width, (int)simg.height);
                node.cameraInfoCallback(cam);
                CHECK(node.imageCallback(simg, &s1) && s1.array_published && s1.array.detections.size() == s0.array.detections.size());
            }
            CHECK(s1.markers.size() == s0.markers.size() && s1.tf.size() == s0.tf.size());
            Stag stag(sp.libraryHD, sp.errorCorrection, false, argv[4], (int)simg.width, (int)simg.height, 0);
            stag.detectMarkers(simg.data.data(), (int)simg.width, (int)simg.height, (int)simg.step);
            std::vector<fid_pose_cov> scov;
            const std::vector<fid_stag_pose_out> sposes = stag.solvePnpSingleCov(camera, (double)sp.marker_size, 0.5, &scov);
            CHECK(sposes.size() == s1.array.detections.size());
            for (size_t i = 0; i < s1.array.detections.size() && i < sposes.size(); i++) {
                const ObjectHypothesisWithPose &hyp = s1.array.detections[i].results[0], &hyp0 = s0.array.detections[i].results[0];
                CHECK(hyp.id == sposes[i].id && samePose(hyp.pose, hyp0.pose) && samePose(s1.markers[i].pose, s0.markers[i].pose));
                CHECK(scov[i].status == 0 && std::memcmp(hyp.covariance.data(), scov[i].cov_pose, sizeof(double) * 36) == 0 && !allZero(hyp.covariance));
            }
        }
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
