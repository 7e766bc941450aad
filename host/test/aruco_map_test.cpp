// aruco_map_test.cpp -- FiducialsNode (host/include/fiducials_host.hpp) with ~map_file: the camera in the map of fiducials.
//   usage: aruco_map_test <frame.pgm> <map.txt> <camera.txt> <data_dir> <dictionary> <fiducial_len>
//   camera.txt: "fx fy cx cy", then "n_mapped" (the markers of the picture that the map names).
// checks that poseEstimateCallback's PoseOutputs carries one PoseStamped, frame_id "map", equal to what fid_map_pose_last gives for
// the same frame on a context of its own (cam_t, cam_R as a quaternion); that everything else the node publishes is what a node
// without a map publishes; that an ignored id leaves the map pose of the remaining markers; and that a map file that cannot be
// read is refused when the node is made.
#include <cmath>
#include <cstdio>
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

static bool sameTransforms(const FiducialTransformArray &a, const FiducialTransformArray &b)
{
    if (a.transforms.size() != b.transforms.size() || a.image_seq != b.image_seq) return false;
    for (size_t i = 0; i < a.transforms.size(); i++) {
        const FiducialTransform &x = a.transforms[i], &y = b.transforms[i];
        if (x.fiducial_id != y.fiducial_id || x.tx != y.tx || x.ty != y.ty || x.tz != y.tz || x.qx != y.qx || x.qy != y.qy || x.qz != y.qz ||
            x.qw != y.qw || x.image_error != y.image_error || x.object_error != y.object_error || x.fiducial_area != y.fiducial_area)
            return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 7) {
        std::printf("usage: %s <frame.pgm> <map.txt> <camera.txt> <data dir> <dictionary> <fiducial_len>\n", argv[0]);
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
        int n_mapped = 0;
        {
            std::ifstream e(argv[3]);
            double fx, fy, cx, cy;
            e >> fx >> fy >> cx >> cy >> n_mapped;
            cam.K = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
            cam.D = {0.05, -0.02, 0.001, -0.0005, 0};
        }
        FiducialsNode::Params p;
        p.data_dir = argv[4];
        p.dictionary = std::atoi(argv[5]);
        p.fiducial_len = std::atof(argv[6]);
        p.max_width = w;
        p.max_height = h;
        // ---- no map: nothing extra
        FiducialsNode plain(p);
        plain.camInfoCallback(cam);
        FiducialArray fa0;
        PoseOutputs o0;
        CHECK(plain.imageCallback(img, &fa0) && plain.poseEstimateCallback(fa0, &o0));
        CHECK(o0.map_pose.empty() && !o0.fta.transforms.empty());
        // ---- a map file that is not there is refused when the node is made
        bool threw = false;
        try {
            FiducialsNode::Params bad = p;
            bad.map_file = std::string(argv[2]) + ".nowhere";
            FiducialsNode node(bad);
        } catch (const std::runtime_error &) {
            threw = true;
        }
        CHECK(threw);
        // ---- the map from the file
        p.map_file = argv[2];
        FiducialsNode node(p);
        node.camInfoCallback(cam);
        FiducialArray fa;
        PoseOutputs out;
        for (int round = 0; round < 2; round++) {  // (the second frame: the detect call has posed the camera already)
            CHECK(node.imageCallback(img, &fa) && node.poseEstimateCallback(fa, &out));
            CHECK(fa.fiducials.size() == fa0.fiducials.size());
            CHECK(sameTransforms(out.fta, o0.fta) && out.tf.size() == o0.tf.size());
            CHECK(out.map_pose.size() == 1);
        }
        // the same frame through the C interface on a context of its own
        std::vector<fid_map_entry> entries(FID_MAP_MAX_ENTRIES);
        int32_t n_entries = 0, skipped = 0;
        CHECK(fid_map_load_file(argv[2], p.fiducial_len, entries.data(), (int32_t)entries.size(), &n_entries, &skipped) == FID_OK && skipped == 1);
        Dictionary dict = getPredefinedDictionary(p.dictionary, p.data_dir);
        fid_dict fd = dict.view();
        fid_limits lim;
        fid_default_limits(&lim);
        lim.max_width = w; lim.max_height = h; lim.max_batch = 1;
        fid_ctx *ctx = nullptr;
        CHECK(fid_create(&p.detector, &fd, &lim, 0, &ctx) == FID_OK);
        std::vector<fid_marker> mk(1024);
        int32_t n = 0;
        fid_map_pose_out want;
        double D5[5] = {cam.D[0], cam.D[1], cam.D[2], cam.D[3], cam.D[4]};
        CHECK(fid_set_map(ctx, entries.data(), n_entries) == FID_OK);
        CHECK(fid_detect(ctx, img.data.data(), w, h, w, FID_ENC_MONO8, mk.data(), (int32_t)mk.size(), &n) == FID_OK);
        CHECK(fid_map_pose_last(ctx, cam.K.data(), D5, &want, 1) == FID_OK && want.n_markers == n_mapped);
        if (out.map_pose.size() == 1) {
            const PoseStamped &ps = out.map_pose[0];
            CHECK(ps.header.frame_id == "map" && ps.header.sec == 55 && ps.header.nsec == 3);
            CHECK(ps.pose.px == want.cam_t[0] && ps.pose.py == want.cam_t[1] && ps.pose.pz == want.cam_t[2]);
            // the quaternion is cam_R
            const double x = ps.pose.ox, y = ps.pose.oy, z = ps.pose.oz, qw = ps.pose.ow;
            const double Rq[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * qw), 2 * (x * z + y * qw), 2 * (x * y + z * qw), 1 - 2 * (x * x + z * z),
                                  2 * (y * z - x * qw), 2 * (x * z - y * qw), 2 * (y * z + x * qw), 1 - 2 * (x * x + y * y)};
            for (int i = 0; i < 9; i++) CHECK(std::fabs(Rq[i] - want.cam_R[i]) < 1e-12);
            CHECK(std::fabs(x * x + y * y + z * z + qw * qw - 1.0) < 1e-12);
        }
        // ---- an ignored id: the pose of the markers that are left
        if (n_mapped >= 2 && !fa.fiducials.empty()) {
            const int gone = fa.fiducials[0].fiducial_id;
            std::vector<fid_marker> kept;
            for (int i = 0; i < n; i++)
                if (mk[(size_t)i].id != gone) kept.push_back(mk[(size_t)i]);
            fid_map_pose_out rest;
            CHECK(fid_map_pose(ctx, cam.K.data(), D5, kept.data(), (int32_t)kept.size(), &rest) == FID_OK && rest.n_markers == n_mapped - 1);
            node.ignoreCallback(std::to_string(gone));
            PoseOutputs oi;
            CHECK(node.imageCallback(img, &fa) && node.poseEstimateCallback(fa, &oi) && oi.map_pose.size() == 1);
            if (oi.map_pose.size() == 1)
                CHECK(oi.map_pose[0].pose.px == rest.cam_t[0] && oi.map_pose[0].pose.py == rest.cam_t[1] && oi.map_pose[0].pose.pz == rest.cam_t[2]);
        }
        fid_destroy(ctx);
    } catch (const std::exception &e) {
        std::printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    std::printf(g_fail ? "%d check(s) failed\n" : "all checks passed%.0d\n", g_fail);
    return g_fail ? 1 : 0;
}
