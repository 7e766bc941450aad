// camera_models_test.cpp -- FiducialsNode (host/include/fiducials_host.hpp) under the camera models of CameraInfo.distortion_model.
//   usage: camera_models_test <frame.pgm> <camera.txt> <data_dir> <dictionary> <fiducial_len>
//   camera.txt: "fx fy cx cy".  The frame is rendered with the plain pinhole.
// checks that a rational_polynomial CameraInfo with eight zero coefficients gives the transforms of the plumb-bob node (equal, not
// close); that an equidistant one with four zero coefficients -- the ideal fisheye r_d = theta, which is no pinhole -- and a
// rational one with a depth camera's coefficients give transforms that differ from the plumb-bob node's and are fid_pose_cam's for
// the same camera; and that a 14-coefficient model with a tilted sensor publishes vertices and no transforms, and says why.
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

// the node's transforms against fid_pose_cam on the vertices it published, on a context of its own
static void checkAgainstPoseCam(fid_ctx *ctx, const fid_camera &camera, const FiducialArray &fa, const FiducialTransformArray &fta, double len)
{
    const int n = (int)fa.fiducials.size();
    std::vector<fid_marker> mk((size_t)n);
    for (int i = 0; i < n; i++) {
        const Fiducial &f = fa.fiducials[(size_t)i];
        mk[(size_t)i].id = f.fiducial_id;
        const double c[8] = {f.x0, f.y0, f.x1, f.y1, f.x2, f.y2, f.x3, f.y3};
        for (int k = 0; k < 8; k++) mk[(size_t)i].corners[k] = (float)c[k];
    }
    std::vector<fid_pose_out> poses((size_t)(n > 0 ? n : 1));
    CHECK(fid_pose_cam(ctx, &camera, mk.data(), nullptr, n, len, poses.data()) == FID_OK);
    CHECK((int)fta.transforms.size() == n);
    for (int i = 0; i < n && i < (int)fta.transforms.size(); i++) {
        const FiducialTransform &t = fta.transforms[(size_t)i];
        const fid_pose_out &p = poses[(size_t)i];
        CHECK(t.fiducial_id == mk[(size_t)i].id);
        CHECK(t.tx == p.tvec[0] && t.ty == p.tvec[1] && t.tz == p.tvec[2]);
        CHECK(t.image_error == p.image_error && t.object_error == p.object_error && t.fiducial_area == p.fiducial_area);
        const double angle = std::sqrt(p.rvec[0] * p.rvec[0] + p.rvec[1] * p.rvec[1] + p.rvec[2] * p.rvec[2]);
        CHECK(std::fabs(t.qw - std::cos(angle * 0.5)) < 1e-12);
        CHECK(std::fabs(t.qx - p.rvec[0] / angle * std::sin(angle * 0.5)) < 1e-12);
    }
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::printf("usage: %s <frame.pgm> <camera.txt> <data dir> <dictionary> <fiducial_len>\n", argv[0]);
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
        img.header.seq = 4; img.header.sec = 21; img.header.nsec = 8; img.header.frame_id = "camera";
        img.data.resize((size_t)w * h);
        f.read((char *)img.data.data(), (std::streamsize)img.data.size());
        CameraInfo cam;
        cam.header.frame_id = "camera";
        {
            std::ifstream e(argv[2]);
            double fx, fy, cx, cy;
            e >> fx >> fy >> cx >> cy;
            cam.K = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
        }
        FiducialsNode::Params p;
        p.data_dir = argv[3];
        p.dictionary = std::atoi(argv[4]);
        p.fiducial_len = std::atof(argv[5]);
        p.max_width = w;
        p.max_height = h;
        auto run = [&](const char *model, const std::vector<double> &D, FiducialArray *fa, PoseOutputs *out, std::string *err) {
            FiducialsNode node(p);
            CameraInfo ci = cam;
            ci.distortion_model = model;
            ci.D = D;
            node.camInfoCallback(ci);
            bool posed = false;
            for (int frame = 0; frame < 7; frame++) {  // ("No camera intrinsics" is reported from the sixth frame on)
                CHECK(node.imageCallback(img, fa));
                *out = PoseOutputs();
                posed = node.poseEstimateCallback(*fa, out);
            }
            *err = node.lastError();
            return posed;
        };
        FiducialArray fa0, fa;
        PoseOutputs o0, o;
        std::string err;
        // ---- the plumb-bob node
        CHECK(run("plumb_bob", {0, 0, 0, 0, 0}, &fa0, &o0, &err));
        CHECK(fa0.fiducials.size() >= 3 && o0.fta.transforms.size() == fa0.fiducials.size());
        // a context of its own for fid_pose_cam
        Dictionary dict = getPredefinedDictionary(p.dictionary, p.data_dir);
        fid_dict fd = dict.view();
        fid_limits lim;
        fid_default_limits(&lim);
        lim.max_width = w; lim.max_height = h; lim.max_batch = 1;
        fid_ctx *ctx = nullptr;
        CHECK(fid_create(&p.detector, &fd, &lim, 0, &ctx) == FID_OK);
        fid_camera camera;
        // ---- rational_polynomial with eight zero coefficients: the plumb-bob node's transforms
        CHECK(run("rational_polynomial", std::vector<double>(8, 0.0), &fa, &o, &err));
        CHECK(fa.fiducials.size() == fa0.fiducials.size() && sameTransforms(o.fta, o0.fta));
        // ---- equidistant with four zero coefficients goes through the fisheye kernel: fid_pose_cam's transforms for that camera
        CHECK(run("equidistant", std::vector<double>(4, 0.0), &fa, &o, &err));
        CHECK(fid_camera_from_info("equidistant", cam.K.data(), std::vector<double>(4, 0.0).data(), 4, &camera) == FID_OK && camera.model == FID_CAM_EQUIDISTANT);
        CHECK(fa.fiducials.size() == fa0.fiducials.size() && !sameTransforms(o.fta, o0.fta));
        checkAgainstPoseCam(ctx, camera, fa, o.fta, p.fiducial_len);
        // ---- a depth camera's rational coefficients: other transforms than the plumb-bob node's, fid_pose_cam's
        const std::vector<double> kinect = {0.4319, -2.7146, 0.00052, -0.00031, 1.6045, 0.3122, -2.5286, 1.5265};
        CHECK(run("rational_polynomial", kinect, &fa, &o, &err));
        CHECK(fid_camera_from_info("rational_polynomial", cam.K.data(), kinect.data(), 8, &camera) == FID_OK && camera.model == FID_CAM_RATIONAL);
        CHECK(fa.fiducials.size() == fa0.fiducials.size() && !sameTransforms(o.fta, o0.fta));
        checkAgainstPoseCam(ctx, camera, fa, o.fta, p.fiducial_len);
        // ---- a tilted sensor: vertices, no transforms, and the reason
        std::vector<double> tilted(14, 0.0);
        tilted[12] = 0.01;
        CHECK(!run("rational_polynomial", tilted, &fa, &o, &err));
        CHECK(fa.fiducials.size() == fa0.fiducials.size() && o.fta.transforms.empty() && o.tf.empty());
        CHECK(err.find("No camera intrinsics") == 0 && err.find("tilted") != std::string::npos);
        // ---- a model nobody knows: the same
        CHECK(!run("double_sphere", {0, 0, 0, 0, 0, 0}, &fa, &o, &err));
        CHECK(o.fta.transforms.empty() && err.find("double_sphere") != std::string::npos);
        fid_destroy(ctx);
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
