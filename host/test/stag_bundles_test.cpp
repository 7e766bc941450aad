// stag_bundles_test.cpp -- StagNode (host/include/stag_host.hpp) with a layout: bundles and standalone tags of a written-out scene.
//   usage: stag_bundles_test <frame.pgm> <layout.yaml> <expected.txt> <data_dir> <hd> <errorCorrection>
//   expected.txt: "fx fy cx cy", then "n_bundles", then per bundle of the YAML "frame standalone tx ty tz" (the rendered translation;
//   standalone = 1 for an entry of `tags:`), then "n_loose" and that many ids the layout does not name.
// checks the bundle PoseStamped (frame names, rendered distance), TF, that members of a multi-tag bundle are absent from the per-marker
// outputs, that a standalone tag is published under its frame from its own corners, that ids outside the layout keep the marker_size
// pose, and that a node without a layout publishes what it always has.
#include <cstdio>
#include <fstream>
#include <iostream>

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

static bool samePose(const Pose &a, const Pose &b)
{
    return a.px == b.px && a.py == b.py && a.pz == b.pz && a.ox == b.ox && a.oy == b.oy && a.oz == b.oz && a.ow == b.ow;
}

int main(int argc, char **argv)
{
    if (argc < 7) {
        std::printf("usage: %s <frame.pgm> <layout.yaml> <expected.txt> <data dir> <hd> <errorCorrection>\n", argv[0]);
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
        struct Exp { std::string frame; int standalone; double t[3]; };
        std::vector<Exp> exp;
        std::vector<int> loose;
        CameraInfo cam;
        cam.header.frame_id = "camera";
        {
            std::ifstream e(argv[3]);
            double fx, fy, cx, cy;
            e >> fx >> fy >> cx >> cy;
            cam.K = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
            cam.D = {0, 0, 0, 0, 0};
            int n;
            e >> n;
            exp.resize((size_t)n);
            for (auto &x : exp) e >> x.frame >> x.standalone >> x.t[0] >> x.t[1] >> x.t[2];
            e >> n;
            loose.resize((size_t)n);
            for (int &v : loose) e >> v;
        }
        StagNode::Params p;
        p.libraryHD = std::atoi(argv[5]);
        p.errorCorrection = std::atoi(argv[6]);
        p.marker_size = 0.08f;
        p.publish_tf = true;
        p.tag_tf_prefix = "STag_";
        // ---- no layout: today's outputs
        StagNode plain(p, argv[4], w, h);
        StagNode::Outputs o0;
        plain.cameraInfoCallback(cam);
        CHECK(plain.imageCallback(img, &o0) && o0.bundles.empty());
        const std::vector<Marker> markers = plain.lastMarkers();
        CHECK(o0.markers.size() == markers.size() && o0.tf.size() == markers.size() && o0.array.detections.size() == markers.size());
        for (size_t i = 0; i < o0.markers.size() && i < markers.size(); i++)
            CHECK(o0.markers[i].header.frame_id == std::to_string(markers[i].id) && o0.tf[i].child_frame_id == "STag_" + std::to_string(markers[i].id));
        // ---- a malformed layout file is refused when the node is made
        bool threw = false;
        try {
            StagNode::Params bad = p;
            bad.layout_file = argv[1];  // (the picture is no YAML)
            StagNode node(bad, argv[4], w, h);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        CHECK(threw);
        // ---- the layout from the YAML file
        p.layout_file = argv[2];
        StagNode node(p, argv[4], w, h);
        CHECK(node.params.layout_frames.size() == exp.size());
        for (size_t b = 0; b < exp.size() && b < node.params.layout_frames.size(); b++)
            CHECK(node.params.layout_frames[b] == exp[b].frame && (int)node.params.layout_standalone[b] == exp[b].standalone);
        StagNode::Outputs out;
        node.cameraInfoCallback(cam);
        CHECK(node.imageCallback(img, &out) && out.array_published);
        auto member = [&](int id) {
            for (const fid_stag_tag &t : node.params.layout_tags)
                if (t.id == id) return (int)t.bundle;
            return -1;
        };
        // the per-marker outputs: everything but the members of multi-tag bundles, in marker order
        size_t k = 0;
        for (size_t i = 0; i < markers.size(); i++) {
            const int b = member(markers[i].id);
            if (b >= 0 && !exp[(size_t)b].standalone) continue;
            CHECK(k < out.markers.size());
            if (k >= out.markers.size()) break;
            const std::string want = b >= 0 ? exp[(size_t)b].frame : std::to_string(markers[i].id);
            CHECK(out.markers[k].header.frame_id == want && out.markers[k].header.sec == 55);
            CHECK(out.array.detections[k].results[0].id == markers[i].id && samePose(out.array.detections[k].results[0].pose, out.markers[k].pose));
            CHECK(out.tf[k].child_frame_id == "STag_" + want && out.tf[k].header.frame_id == "camera" && out.tf[k].tz == out.markers[k].pose.pz);
            if (b < 0) {
                CHECK(samePose(out.markers[k].pose, o0.markers[i].pose));  // an id the layout does not name: the marker_size pose
            } else {
                const double *t = exp[(size_t)b].t;
                const Pose &q = out.markers[k].pose;
                const double d = std::sqrt((q.px - t[0]) * (q.px - t[0]) + (q.py - t[1]) * (q.py - t[1]) + (q.pz - t[2]) * (q.pz - t[2]));
                CHECK(d < 0.02 * std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]));  // from its own corners: the rendered place
            }
            k++;
        }
        CHECK(k == out.markers.size() && out.array.detections.size() == k);
        size_t n_loose_seen = 0;
        for (int id : loose)
            for (const PoseStamped &m : out.markers) n_loose_seen += m.header.frame_id == std::to_string(id);
        CHECK(n_loose_seen == loose.size());
        // the bundles: one PoseStamped per multi-tag bundle, in bundle order, at the rendered place; TF behind the markers' TF
        size_t nb = 0;
        for (size_t b = 0; b < exp.size(); b++) {
            if (exp[b].standalone) continue;
            CHECK(nb < out.bundles.size());
            if (nb >= out.bundles.size()) break;
            const PoseStamped &ps = out.bundles[nb];
            CHECK(ps.header.frame_id == exp[b].frame && ps.header.sec == 55 && ps.header.nsec == 3);
            const double *t = exp[b].t;
            const double d = std::sqrt((ps.pose.px - t[0]) * (ps.pose.px - t[0]) + (ps.pose.py - t[1]) * (ps.pose.py - t[1]) + (ps.pose.pz - t[2]) * (ps.pose.pz - t[2]));
            CHECK(d < 0.02 * std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]));
            CHECK(std::fabs(ps.pose.ox * ps.pose.ox + ps.pose.oy * ps.pose.oy + ps.pose.oz * ps.pose.oz + ps.pose.ow * ps.pose.ow - 1.0) < 1e-9);
            CHECK(k + nb < out.tf.size() && out.tf[k + nb].child_frame_id == "STag_" + exp[b].frame && out.tf[k + nb].tz == ps.pose.pz &&
                  out.tf[k + nb].header.frame_id == "camera");
            nb++;
        }
        CHECK(nb == out.bundles.size() && out.tf.size() == k + nb && nb >= 1);
        // the same layout set in code
        StagNode::Params pc = p;
        pc.layout_file.clear();
        pc.layout_tags = node.params.layout_tags;
        pc.layout_frames = node.params.layout_frames;
        pc.layout_standalone = node.params.layout_standalone;
        StagNode coded(pc, argv[4], w, h);
        StagNode::Outputs oc;
        coded.cameraInfoCallback(cam);
        CHECK(coded.imageCallback(img, &oc) && oc.bundles.size() == out.bundles.size() && oc.markers.size() == out.markers.size());
        for (size_t i = 0; i < oc.bundles.size() && i < out.bundles.size(); i++) CHECK(samePose(oc.bundles[i].pose, out.bundles[i].pose));
    } catch (const std::exception &e) {
        std::printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    std::printf(g_fail ? "%d check(s) failed\n" : "all checks passed%.0d\n", g_fail);
    return g_fail ? 1 : 0;
}
