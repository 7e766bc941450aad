// stag_host.hpp -- the host side of the stag_detect drop-in in the reference's language: class Stag with the constructor and
// the two calls StagNode uses (stag_detect/include/stag/Stag.h:41-45), on top of fid_stag_* (include/fid_abi.h), and the
// message step of StagNode::imageCallback (stag_detect.cpp:110-217) producing the fiducial_msgs contract north_star asks for
// (vertices + transforms) instead of PoseStamped / Detection2DArray.  Header-only; no OpenCV: images are (pointer, cols, rows,
// step) and points are plain structs.
#ifndef STAG_HOST_HPP
#define STAG_HOST_HPP
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "fid_abi.h"
#include "fiducials_host.hpp"

namespace fiducials_amd {

struct Point2d {
    double x = 0, y = 0;
};

struct Marker {  // stag/Marker.h + Quad.h: what getMarkerList() hands out
    int id = 0;
    std::vector<Point2d> corners;  // 4, clockwise from the marker's first corner
    Point2d center;
    double H[9] = {0};
    double projectiveDistortion = 0;
};

class Stag {
   public:
    // Stag(int libraryHD = 15, int errorCorrection = 7, bool keepLogs = false); data_dir holds stag_HD<hd>.bin (the published
    // marker libraries, tools/make_stag_libraries.py).  Throws std::invalid_argument for an invalid library like Decoder does.
    Stag(int libraryHD = 15, int inErrorCorrection = 7, bool /*inKeepLogs*/ = false, const std::string &data_dir = "fiducials_amd/data",
         int max_width = 1920, int max_height = 1080, int device = 0)
    {
        if (libraryHD < 11 || libraryHD > 23 || !(libraryHD & 1))
            throw std::invalid_argument("Invalid library HD. Possible values are 11, 13, 15, 17, 19, 21, or 23");
        std::ifstream f(data_dir + "/stag_HD" + std::to_string(libraryHD) + ".bin", std::ios::binary);
        if (!f) throw std::runtime_error("marker library not found under " + data_dir);
        f.seekg(0, std::ios::end);
        words.resize((size_t)f.tellg() / 8);
        f.seekg(0);
        f.read((char *)words.data(), (std::streamsize)words.size() * 8);
        fid_status rc = fid_stag_create(libraryHD, inErrorCorrection, max_width, max_height, device, &ctx);
        if (rc == FID_OK) rc = fid_stag_load_library(ctx, words.data(), (int32_t)words.size());
        if (rc != FID_OK) {
            fid_stag_destroy(ctx);
            throw std::runtime_error(std::string("fid_stag_create: ") + fid_strerror(rc));
        }
    }
    ~Stag() { fid_stag_destroy(ctx); }
    Stag(const Stag &) = delete;
    Stag &operator=(const Stag &) = delete;

    // void detectMarkers(cv::Mat inImage): a mono8 image
    void detectMarkers(const uint8_t *data, int cols, int rows, int step)
    {
        std::vector<fid_stag_marker> m(256);
        int32_t n = 0;
        fid_status rc = fid_stag_detect_markers(ctx, data, cols, rows, step, m.data(), (int32_t)m.size(), &n);
        if (rc == FID_E_CAPACITY) {
            m.resize((size_t)n);
            rc = fid_stag_detect_markers(ctx, data, cols, rows, step, m.data(), (int32_t)m.size(), &n);
        }
        if (rc != FID_OK) throw std::runtime_error(std::string("fid_stag_detect_markers: ") + fid_strerror(rc));
        setMarkers(m, n);
    }
    // the same on a frame in device memory of this context's device (a decoded JPEG: fid_jpeg_device_ptr; mono8, bgr8 or rgb8,
    // colour in the 15-bit gray form, include/fid_abi.h)
    void detectMarkersDevice(const void *d_data, int cols, int rows, int step, fid_encoding enc = FID_ENC_MONO8)
    {
        std::vector<fid_stag_marker> m(256);
        int32_t n = 0;
        fid_status rc = fid_stag_detect_markers_device(ctx, d_data, cols, rows, step, enc, m.data(), (int32_t)m.size(), &n);
        if (rc == FID_E_CAPACITY) {
            m.resize((size_t)n);
            rc = fid_stag_detect_markers_device(ctx, d_data, cols, rows, step, enc, m.data(), (int32_t)m.size(), &n);
        }
        if (rc != FID_OK) throw std::runtime_error(std::string("fid_stag_detect_markers_device: ") + fid_strerror(rc));
        setMarkers(m, n);
    }
    std::vector<Marker> getMarkerList() const { return markers; }

    // Common::solvePnpSingle for the markers of the last detectMarkers() (stag_detect.cpp:140-165)
    std::vector<fid_stag_pose_out> solvePnpSingle(const double K[9], const double D[5], double marker_size)
    {
        const fid_camera cam = plumbBob(K, D);
        return solvePnpSingle(cam, marker_size);
    }
    // ... under any camera model the library knows (fid_camera)
    std::vector<fid_stag_pose_out> solvePnpSingle(const fid_camera &cam, double marker_size)
    {
        std::vector<fid_stag_pose_out> p(markers.empty() ? 1 : markers.size());
        int32_t n = 0;
        const fid_status rc = fid_stag_pose_last_cam(ctx, &cam, marker_size, p.data(), (int32_t)p.size(), &n);
        if (rc != FID_OK) throw std::runtime_error(std::string("fid_stag_pose_last: ") + fid_strerror(rc));
        p.resize((size_t)n);
        return p;
    }
    // ... with the covariance of every pose (fid_stag_pose_last_cov_cam; sigma_px 0: a-posteriori); the poses are solvePnpSingle's
    std::vector<fid_stag_pose_out> solvePnpSingleCov(const fid_camera &cam, double marker_size, double sigma_px, std::vector<fid_pose_cov> *cov)
    {
        std::vector<fid_stag_pose_out> p(markers.empty() ? 1 : markers.size());
        cov->assign(p.size(), fid_pose_cov());
        int32_t n = 0;
        const fid_status rc = fid_stag_pose_last_cov_cam(ctx, &cam, marker_size, p.data(), (int32_t)p.size(), &n, sigma_px, cov->data());
        if (rc != FID_OK) throw std::runtime_error(std::string("fid_stag_pose_last_cov: ") + fid_strerror(rc));
        p.resize((size_t)n);
        cov->resize((size_t)n);
        return p;
    }
    // {FID_CAM_PLUMB_BOB, 5, K, D}
    static fid_camera plumbBob(const double K[9], const double D[5])
    {
        fid_camera cam = {};
        cam.model = FID_CAM_PLUMB_BOB;
        cam.n_dist = 5;
        for (int i = 0; i < 9; i++) cam.K[i] = K[i];
        for (int i = 0; i < 5; i++) cam.D[i] = D ? D[i] : 0.0;
        return cam;
    }

    // the node's `bundles` and `tags` (stag_nodelet.h:90-91) on the device; an empty list clears them
    void setLayout(const std::vector<fid_stag_tag> &tags, int n_bundles)
    {
        const fid_status rc = fid_stag_set_layout(ctx, tags.empty() ? nullptr : tags.data(), (int32_t)tags.size(), n_bundles);
        if (rc != FID_OK) throw std::runtime_error(std::string("fid_stag_set_layout: ") + fid_strerror(rc));
    }
    // Common::solvePnpBundle (common.hpp:48-59) for the markers of the last detectMarkers(): one record per bundle that was seen
    std::vector<fid_stag_bundle_pose_out> solvePnpBundle(const double K[9], const double D[5])
    {
        const fid_camera cam = plumbBob(K, D);
        return solvePnpBundle(cam);
    }
    std::vector<fid_stag_bundle_pose_out> solvePnpBundle(const fid_camera &cam)
    {
        std::vector<fid_stag_bundle_pose_out> p(FID_STAG_MAX_BUNDLES);
        int32_t n = 0;
        const fid_status rc = fid_stag_bundle_pose_last_cam(ctx, &cam, p.data(), (int32_t)p.size(), &n);
        if (rc != FID_OK) throw std::runtime_error(std::string("fid_stag_bundle_pose_last: ") + fid_strerror(rc));
        p.resize((size_t)n);
        return p;
    }
    std::vector<fid_stag_bundle_pose_out> solvePnpBundleCov(const fid_camera &cam, double sigma_px, std::vector<fid_pose_cov> *cov)
    {
        std::vector<fid_stag_bundle_pose_out> p(FID_STAG_MAX_BUNDLES);
        cov->assign(p.size(), fid_pose_cov());
        int32_t n = 0;
        const fid_status rc = fid_stag_bundle_pose_last_cov_cam(ctx, &cam, p.data(), (int32_t)p.size(), &n, sigma_px, cov->data());
        if (rc != FID_OK) throw std::runtime_error(std::string("fid_stag_bundle_pose_last_cov: ") + fid_strerror(rc));
        p.resize((size_t)n);
        cov->resize((size_t)n);
        return p;
    }

   private:
    void setMarkers(const std::vector<fid_stag_marker> &m, int32_t n)
    {
        markers.clear();
        for (int i = 0; i < n; i++) {
            Marker k;
            k.id = m[i].id;
            k.corners.resize(4);
            for (int c = 0; c < 4; c++) {
                k.corners[c].x = m[i].corners[2 * c];
                k.corners[c].y = m[i].corners[2 * c + 1];
            }
            k.center.x = m[i].center[0];
            k.center.y = m[i].center[1];
            for (int j = 0; j < 9; j++) k.H[j] = m[i].H[j];
            k.projectiveDistortion = m[i].projectiveDistortion;
            markers.push_back(k);
        }
    }
    fid_stag_ctx *ctx = nullptr;
    std::vector<uint64_t> words;
    std::vector<Marker> markers;
};

// tf::Matrix3x3::getRotation (what stag_detect.cpp:171-178 turns the pose matrix into)
inline void rotationToQuaternion(const double m[9], double q[4] /* x y z w */)
{
    const double trace = m[0] + m[4] + m[8];
    double temp[4];
    if (trace > 0.0) {
        double s = std::sqrt(trace + 1.0);
        temp[3] = s * 0.5;
        s = 0.5 / s;
        temp[0] = (m[7] - m[5]) * s;
        temp[1] = (m[2] - m[6]) * s;
        temp[2] = (m[3] - m[1]) * s;
    } else {
        const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double s = std::sqrt(m[3 * i + i] - m[3 * j + j] - m[3 * k + k] + 1.0);
        temp[i] = s * 0.5;
        s = 0.5 / s;
        temp[3] = (m[3 * k + j] - m[3 * j + k]) * s;
        temp[j] = (m[3 * j + i] + m[3 * i + j]) * s;
        temp[k] = (m[3 * k + i] + m[3 * i + k]) * s;
    }
    for (int a = 0; a < 4; a++) q[a] = temp[a];
}

// CameraInfo -> fid_camera.  "plumb_bob" or no model name: D[0..4], zero where the message is shorter, as before the library knew
// other models; any other name: fid_camera_from_info decides, and what it refuses throws with its message (never a plumb-bob pose
// from a camera of another model)
inline fid_camera stagCameraFromInfo(const CameraInfo &msg)
{
    if (msg.distortion_model.empty() || msg.distortion_model == "plumb_bob") {
        double D[5] = {0, 0, 0, 0, 0};
        for (size_t i = 0; i < msg.D.size() && i < 5; i++) D[i] = msg.D[i];
        return Stag::plumbBob(msg.K.data(), D);
    }
    fid_camera cam = {};
    if (fid_camera_from_info(msg.distortion_model.c_str(), msg.K.data(), msg.D.data(), (int32_t)msg.D.size(), &cam) != FID_OK)
        throw std::runtime_error(fid_camera_last_error());
    return cam;
}

// StagNode::imageCallback with the fiducial_msgs contract: vertices + transforms of one image
inline void stagImageCallback(Stag &stag, const Image &msg, const CameraInfo &cam, double marker_size, FiducialArray *fva, FiducialTransformArray *fta)
{
    stag.detectMarkers(msg.data.data(), (int)msg.width, (int)msg.height, (int)msg.step);
    const std::vector<Marker> markers = stag.getMarkerList();
    const std::vector<fid_stag_pose_out> poses = stag.solvePnpSingle(stagCameraFromInfo(cam), marker_size);
    fva->header.sec = fta->header.sec = msg.header.sec;
    fva->header.nsec = fta->header.nsec = msg.header.nsec;
    fva->header.frame_id = fta->header.frame_id = cam.header.frame_id;
    fva->image_seq = fta->image_seq = (int32_t)msg.header.seq;
    fva->fiducials.clear();
    fta->transforms.clear();
    for (size_t i = 0; i < markers.size(); i++) {
        const Marker &m = markers[i];
        Fiducial f;
        f.fiducial_id = m.id;
        f.x0 = m.corners[0].x; f.y0 = m.corners[0].y; f.x1 = m.corners[1].x; f.y1 = m.corners[1].y;
        f.x2 = m.corners[2].x; f.y2 = m.corners[2].y; f.x3 = m.corners[3].x; f.y3 = m.corners[3].y;
        fva->fiducials.push_back(f);
        FiducialTransform t;
        t.fiducial_id = m.id;
        t.tx = poses[i].tvec[0]; t.ty = poses[i].tvec[1]; t.tz = poses[i].tvec[2];
        double q[4];
        rotationToQuaternion(poses[i].R, q);
        t.qx = q[0]; t.qy = q[1]; t.qz = q[2]; t.qw = q[3];
        // area as aruco_detect's calcFiducialArea (Heron on two triangles); the STag node has no error estimates
        auto dist = [](const Point2d &a, const Point2d &b) { return std::sqrt((a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y)); };
        double a1 = dist(m.corners[0], m.corners[1]), b1 = dist(m.corners[0], m.corners[3]), c1 = dist(m.corners[1], m.corners[3]);
        double a2 = dist(m.corners[1], m.corners[2]), b2 = dist(m.corners[2], m.corners[3]), c2 = c1;
        const double s1 = (a1 + b1 + c1) / 2.0, s2 = (a2 + b2 + c2) / 2.0;
        t.fiducial_area = std::sqrt(s1 * (s1 - a1) * (s1 - b1) * (s1 - c1)) + std::sqrt(s2 * (s2 - a2) * (s2 - b2) * (s2 - c2));
        fta->transforms.push_back(t);
    }
}

// ---- the reference's node itself, without ROS: StagNode of stag_detect/src/stag_ros/stag_detect.cpp with the outputs IT
// publishes -- one geometry_msgs/PoseStamped per marker on `stag_ros/markers` (header.frame_id = the marker id as text,
// common.hpp:72-82), one vision_msgs/Detection2DArray on `stag_ros/markers_array` (stag_detect.cpp:139-209; the shipped launch
// remaps it onto /fiducial_transforms, stag_detect.launch:10) and, with `publish_tf`, <image frame> -> <tag_tf_prefix><id>.
// ros/stag_detect_amd is the catkin glue around this class; host/test/stag_test.cpp runs it on the GPU box.
class StagNode {
   public:
    struct Params {  // StagNode::loadParameters (stag_detect.cpp:88-108) with its defaults
        int libraryHD = 15, errorCorrection = 7;
        std::string raw_image_topic = "image_raw", camera_info_topic = "camera_info";
        std::string markers_topic = "stag_ros/markers", markers_array_topic = "stag_ros/markers_array";
        bool is_compressed = false, show_markers = true, publish_tf = false;
        std::string tag_tf_prefix = "STag_";
        float marker_size = 0.18f;
        // the layout (loadTagsBundles, load_yaml_tags.h:75-105): the YAML file that holds `tags:` / `bundles:`, or the tags set in
        // code -- layout_tags with, per bundle, its frame name and whether it is a standalone tag of the `tags:` list.  Neither: no
        // layout, the node publishes what it always has.
        std::string layout_file;
        std::vector<fid_stag_tag> layout_tags;
        std::vector<std::string> layout_frames;
        std::vector<uint8_t> layout_standalone;
        std::string bundles_topic = "stag_ros/bundles";
        // fill ObjectHypothesisWithPose::covariance of `array` with the pose's covariance (fid_abi.h, "pose covariance": cov_pose of
        // the pose that is published -- the marker's, or its bundle's for a standalone tag; 36 zeros for a record whose status is not
        // 0); off: every output is what it was
        bool pose_covariance = false;
        double pose_covariance_sigma_px = 1.0;  // the corner noise in pixels; 0: the a-posteriori estimate from the residuals
    };
    struct Outputs {
        std::vector<PoseStamped> markers;  // Common::publishTransform, one message per marker, in marker order
        std::vector<PoseStamped> bundles;  // bundlePub (stag_nodelet.h:73): one per bundle that was seen, header.frame_id = its frame
        Detection2DArray array;
        std::vector<TransformStamped> tf;
        bool array_published = false;  // (the reference returns before markersArrayPub.publish when a pose comes back empty)
    };

    StagNode(const Params &p, const std::string &data_dir = "fiducials_amd/data", int max_width = 1920, int max_height = 1080, int device = 0)
        : params(p), stag(p.libraryHD, p.errorCorrection, false, data_dir, max_width, max_height, device), maxW(max_width), maxH(max_height), dev(device)
    {
        if (!params.layout_file.empty()) {
            int32_t nt = 0, nb = 0;
            fid_status rc = fid_stag_layout_load_file(params.layout_file.c_str(), nullptr, 0, &nt, &nb, nullptr, nullptr, 0);
            if (rc == FID_E_CAPACITY || (rc == FID_OK && nt > 0)) {
                params.layout_tags.resize((size_t)nt);
                params.layout_standalone.assign((size_t)nb, 0);
                std::vector<char> names((size_t)nb * FID_STAG_FRAME_LEN);
                rc = fid_stag_layout_load_file(params.layout_file.c_str(), params.layout_tags.data(), nt, &nt, &nb, params.layout_standalone.data(),
                                               names.data(), nb);
                params.layout_frames.clear();
                for (int b = 0; b < nb; b++) params.layout_frames.push_back(std::string(names.data() + (size_t)b * FID_STAG_FRAME_LEN));
            }
            if (rc != FID_OK) throw std::invalid_argument(std::string("layout: ") + fid_stag_layout_last_error());
        }
        if (!params.layout_tags.empty()) {
            if (params.layout_standalone.size() != params.layout_frames.size()) throw std::invalid_argument("layout: a frame name and a standalone flag per bundle");
            for (const fid_stag_tag &t : params.layout_tags)
                if (t.bundle < 0 || (size_t)t.bundle >= params.layout_frames.size()) throw std::invalid_argument("layout: bundle index without a frame name");
            stag.setLayout(params.layout_tags, (int)params.layout_frames.size());
        }
    }
    ~StagNode()
    {
        if (jctx) fid_jpeg_destroy(jctx);
        if (ectx) fid_jpeg_enc_destroy(ectx);
    }

    // StagNode::cameraInfoCallback (:219-263): the first message is kept, later ones are ignored
    void cameraInfoCallback(const CameraInfo &msg)
    {
        if (got_camera_info) return;
        try {
            camera = stagCameraFromInfo(msg);
        } catch (const std::runtime_error &e) {  // a model the library does not pose under: as if no CameraInfo had come, said why
            last_error = std::string("No camera intrinsics: ") + e.what();
            return;
        }
        for (int i = 0; i < 9; i++) K[i] = camera.K[i];
        for (int i = 0; i < 5; i++) D[i] = camera.model == FID_CAM_EQUIDISTANT ? 0.0 : camera.D[i];
        got_camera_info = true;
    }

    // stag_ros::msgToGray (utility.hpp:8-20): bgr8 / rgb8 through cvtColor's 8-bit fixed point, mono8 as it is; anything else:
    // false (the reference goes on with an EMPTY image there; this node drops the frame)
    static bool msgToGray(const Image &msg, std::vector<uint8_t> *gray, const uint8_t **data, int *step)
    {
        if (msg.encoding == "mono8") {
            if (msg.step < msg.width || msg.data.size() < (size_t)msg.step * msg.height) return false;
            *data = msg.data.data();
            *step = (int)msg.step;
            return true;
        }
        const bool bgr = msg.encoding == "bgr8", rgb = msg.encoding == "rgb8";
        if (!bgr && !rgb) return false;
        if (msg.step < 3 * msg.width || msg.data.size() < (size_t)msg.step * msg.height) return false;
        gray->resize((size_t)msg.width * msg.height);
        for (uint32_t y = 0; y < msg.height; y++) {
            const uint8_t *s = msg.data.data() + (size_t)y * msg.step;
            uint8_t *o = gray->data() + (size_t)y * msg.width;
            for (uint32_t x = 0; x < msg.width; x++) {
                const int c0 = s[3 * x], g = s[3 * x + 1], c2 = s[3 * x + 2];
                const int b = bgr ? c0 : c2, r = bgr ? c2 : c0;
                o[x] = (uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14);  // imgproc color_rgb: RGB2Gray<uchar>, 14-bit coefficients
            }
        }
        *data = gray->data();
        *step = (int)msg.width;
        return true;
    }

    // StagNode::imageCallback (:110-217).  false: nothing is published (no CameraInfo yet, or an encoding msgToGray refuses).
    bool imageCallback(const Image &msg, Outputs *out)
    {
        out->markers.clear();
        out->bundles.clear();
        out->tf.clear();
        out->array = Detection2DArray();
        out->array_published = false;
        if (!got_camera_info) return false;
        const uint8_t *data = nullptr;
        int step = 0;
        if (!msgToGray(msg, &gray_, &data, &step)) return false;
        stag.detectMarkers(data, (int)msg.width, (int)msg.height, step);
        publishMarkers(msg.header, out);
        return true;
    }

    // the same callback for a frame that arrives compressed (the shipped cfg/single.yaml: is_compressed, the node then subscribes
    // to <raw_image_topic>/compressed).  What the subscriber plugin's cv::imdecode hands to msgToGray, made gray the way
    // cvtColor(BGR2GRAY) does in OpenCV 4.x (15-bit form): a JPEG is decoded ON THE DEVICE (fid_jpeg_decode, MONO8) and detected
    // where it lies (fid_stag_detect_markers_device); a PNG is decoded on the host (fid_png_decode, MONO8) and goes the host road.
    // false: nothing is published (no CameraInfo yet, or a frame that cannot be decoded: the plugin drops those).
    bool compressedImageCallback(const CompressedImage &msg, Outputs *out) { return compressedImageCallback(msg, out, nullptr); }
    // ... and the image the reference publishes on stag_ros/image_markers for every frame when show_markers is set (:123-133):
    // Stag::drawMarkers() draws on the detector's GRAY image expanded to BGR (Drawer.cpp:123-129).  Here: that gray image as bgr8
    // with the marker outlines of fid_draw_detected_markers (cv::line LINE_8; the reference's circles and text are not drawn,
    // include/fid_abi.h) -- made on the device for a JPEG (fid_jpeg_marker_image on the gray already decoded there), on the host
    // for a PNG.  image->data is empty unless an image is published.
    bool compressedImageCallback(const CompressedImage &msg, Outputs *out, Image *image) { return compressedFrame(msg, out, image, nullptr); }
    bool compressedImageCallback(const CompressedImage &msg, Outputs *out, std::nullptr_t) { return compressedFrame(msg, out, nullptr, nullptr); }
    // ... and what stag_ros/image_markers/compressed carries (image_transport offers it for every image publisher): the same image
    // as the JPEG file compressed_image_transport's publisher makes of it (cv::imencode(".jpg")), format "bgr8; jpeg compressed
    // bgr8".  For a JPEG frame it is drawn AND compressed on the device (fid_jpeg_marker_jpeg): only the file crosses to the host;
    // a PNG frame's image is drawn on the host and compressed on the device (fid_jpeg_encode).
    bool compressedImageCallback(const CompressedImage &msg, Outputs *out, CompressedImage *image) { return compressedFrame(msg, out, nullptr, image); }

    const std::vector<Marker> lastMarkers() const { return stag.getMarkerList(); }
    const std::string &lastError() const { return last_error; }

    Params params;
    bool got_camera_info = false;
    double K[9] = {0}, D[5] = {0};  // (the plumb-bob view of `camera`, for callers that read them)
    fid_camera camera = {};

   private:
    bool publishCompressed(const Header &h, const uint8_t *raw, int32_t w, int32_t ht, const std::vector<fid_marker> &mk, CompressedImage *cimage)
    {
        const int64_t room = (int64_t)maxW * maxH * 2 + 65536;  // (a file that needs more is not published)
        if (!ectx) {
            const fid_status rc = fid_jpeg_enc_create(dev, maxW, maxH, 1, room, &ectx);
            if (rc != FID_OK) {
                ectx = nullptr;
                last_error = std::string("fid_jpeg_enc_create: ") + fid_strerror(rc);
                return false;
            }
        }
        cimage->header = h;
        cimage->format = "bgr8; jpeg compressed bgr8";
        cimage->data.resize((size_t)room);
        int64_t nb = 0;
        const fid_status rc = raw ? fid_jpeg_encode(ectx, raw, 1, w, ht, w * 3, 0, FID_ENC_BGR8, cimage->data.data(), room, &nb)
                                  : fid_jpeg_marker_jpeg(jctx, 0, FID_ENC_MONO8, mk.data(), (int32_t)mk.size(), 0, ectx, cimage->data.data(), room, &nb);
        if (rc != FID_OK) {
            last_error = std::string("marker image: ") + fid_strerror(rc) + " (" + (raw ? fid_jpeg_enc_last_error(ectx) : fid_jpeg_last_error(jctx)) + ")";
            cimage->data.clear();
            return false;
        }
        cimage->data.resize((size_t)nb);
        return true;
    }

    bool compressedFrame(const CompressedImage &msg, Outputs *out, Image *image, CompressedImage *cimage)
    {
        if (image) image->data.clear();
        if (cimage) cimage->data.clear();
        Image drawn;  // (a PNG frame's marker image on its way to the encoder)
        if (cimage && !image) image = &drawn;
        out->markers.clear();
        out->bundles.clear();
        out->tf.clear();
        out->array = Detection2DArray();
        out->array_published = false;
        if (!got_camera_info) return false;
        const uint8_t *file = msg.data.data();
        const int64_t nbytes = (int64_t)msg.data.size();
        static const uint8_t png_sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        if (nbytes >= 8 && !std::memcmp(file, png_sig, 8)) {
            fid_png_info pi = {};
            fid_status rc = fid_png_probe(file, nbytes, &pi);
            if (rc != FID_OK || pi.width > maxW || pi.height > maxH) {
                last_error = rc != FID_OK ? std::string("compressed frame: ") + fid_png_last_error() : "compressed frame: larger than the context";
                return false;
            }
            gray_.resize((size_t)pi.width * pi.height);
            rc = fid_png_decode(file, nbytes, FID_ENC_MONO8, gray_.data(), (int64_t)gray_.size(), nullptr);
            if (rc != FID_OK) {
                last_error = std::string("compressed frame: ") + fid_png_last_error();
                return false;
            }
            stag.detectMarkers(gray_.data(), pi.width, pi.height, pi.width);
            publishMarkers(msg.header, out);
            if (params.show_markers && image) {
                startMarkerImage(image, msg.header, pi.width, pi.height);
                const std::vector<fid_marker> mk = markersToDraw();
                fid_status rcd = fid_to_bgr(gray_.data(), pi.width, pi.height, pi.width, FID_ENC_MONO8, image->data.data(), (int64_t)image->data.size());
                if (rcd == FID_OK)
                    rcd = fid_draw_detected_markers(image->data.data(), pi.width, pi.height, (int32_t)image->step, mk.data(), (int32_t)mk.size(), 0);
                if (rcd != FID_OK) {
                    last_error = std::string("marker image: ") + fid_strerror(rcd);
                    image->data.clear();
                }
                if (cimage && !image->data.empty()) publishCompressed(msg.header, image->data.data(), pi.width, pi.height, mk, cimage);
            }
            return true;
        }
        if (!jctx) {
            const fid_status rc = fid_jpeg_create(dev, maxW, maxH, 1, &jctx);
            if (rc != FID_OK) {
                jctx = nullptr;
                last_error = std::string("fid_jpeg_create: ") + fid_strerror(rc);
                return false;
            }
        }
        if (fid_jpeg_decode(jctx, &file, &nbytes, 1, FID_ENC_MONO8, nullptr, 0) != FID_OK) {
            last_error = std::string("compressed frame: ") + fid_jpeg_last_error(jctx);
            return false;
        }
        int32_t w = 0, h = 0, stride = 0;
        int64_t fstride = 0;
        const void *gray = fid_jpeg_device_ptr(jctx, &w, &h, &stride, &fstride);
        stag.detectMarkersDevice(gray, w, h, stride, FID_ENC_MONO8);
        publishMarkers(msg.header, out);
        if (params.show_markers && cimage) {  // drawn and compressed on the device: the raw marker image never crosses to the host
            publishCompressed(msg.header, nullptr, w, h, markersToDraw(), cimage);
            return true;
        }
        if (params.show_markers && image) {
            startMarkerImage(image, msg.header, w, h);
            const std::vector<fid_marker> mk = markersToDraw();
            const fid_status rcd = fid_jpeg_marker_image(jctx, 0, FID_ENC_MONO8, mk.data(), (int32_t)mk.size(), 0, image->data.data(),
                                                         (int64_t)image->data.size());
            if (rcd != FID_OK) {
                last_error = std::string("marker image: ") + fid_strerror(rcd) + " (" + fid_jpeg_last_error(jctx) + ")";
                image->data.clear();
            }
        }
        return true;
    }

    // the markers of the last detection as the drawer takes them (corners cast to float, as the ROS glue does)
    std::vector<fid_marker> markersToDraw() const
    {
        std::vector<fid_marker> mk;
        for (const Marker &m : stag.getMarkerList()) {
            fid_marker k;
            k.id = m.id;
            for (int c = 0; c < 4; c++) {
                k.corners[2 * c] = (float)m.corners[(size_t)c].x;
                k.corners[2 * c + 1] = (float)m.corners[(size_t)c].y;
            }
            mk.push_back(k);
        }
        return mk;
    }
    static void startMarkerImage(Image *image, const Header &h, int32_t w, int32_t ht)
    {
        image->header = h;
        image->height = (uint32_t)ht;
        image->width = (uint32_t)w;
        image->encoding = "bgr8";
        image->is_bigendian = 0;
        image->step = (uint32_t)w * 3;
        image->data.resize((size_t)w * ht * 3);
    }
    // the tail of imageCallback (:133-215): poses of the last detection and everything the node publishes for them
    void publishMarkers(const Header &header, Outputs *out)
    {
        const std::vector<Marker> markers = stag.getMarkerList();
        std::vector<fid_pose_cov> covs, bcovs;
        const std::vector<fid_stag_pose_out> poses = params.pose_covariance
                                                         ? stag.solvePnpSingleCov(camera, (double)params.marker_size, params.pose_covariance_sigma_px, &covs)
                                                         : stag.solvePnpSingle(camera, (double)params.marker_size);
        // with a layout: a member of a multi-tag bundle is not published on its own; a standalone tag of `tags:` is, posed from its
        // own corners and under its own frame; ids the layout does not name keep the marker_size pose
        std::vector<fid_stag_bundle_pose_out> bposes;
        if (!params.layout_tags.empty())
            bposes = params.pose_covariance ? stag.solvePnpBundleCov(camera, params.pose_covariance_sigma_px, &bcovs) : stag.solvePnpBundle(camera);
        auto bundleOf = [this](int id) {  // getTagIndex / getBundleIndex (stag_nodelet.h:59-60)
            for (const fid_stag_tag &t : params.layout_tags)
                if (t.id == id) return (int)t.bundle;
            return -1;
        };
        auto poseOf = [](const double R[9], const double tvec[3]) {
            double q[4];
            rotationToQuaternion(R, q);  // tf::Matrix3x3::getRotation
            Pose pose;
            pose.px = tvec[0]; pose.py = tvec[1]; pose.pz = tvec[2];
            pose.ox = q[0]; pose.oy = q[1]; pose.oz = q[2]; pose.ow = q[3];
            return pose;
        };
        out->array.header = header;
        for (size_t i = 0; i < markers.size(); i++) {
            Pose pose = poseOf(poses[i].R, poses[i].tvec);
            const fid_pose_cov *pcov = params.pose_covariance ? &covs[i] : nullptr;
            std::string id = std::to_string(markers[i].id);
            const int b = bundleOf(markers[i].id);
            if (b >= 0) {
                if (!params.layout_standalone[(size_t)b]) continue;
                for (size_t k = 0; k < bposes.size(); k++)
                    if (bposes[k].bundle == b) {
                        pose = poseOf(bposes[k].R, bposes[k].tvec);
                        if (params.pose_covariance) pcov = &bcovs[k];
                    }
                id = params.layout_frames[(size_t)b];
            }
            if (params.publish_tf) {  // Common::publishTransform: tf first, then the PoseStamped
                TransformStamped t;
                t.header = header;
                t.child_frame_id = params.tag_tf_prefix + id;
                t.tx = pose.px; t.ty = pose.py; t.tz = pose.pz;
                t.qx = pose.ox; t.qy = pose.oy; t.qz = pose.oz; t.qw = pose.ow;
                out->tf.push_back(t);
            }
            PoseStamped ps;
            ps.header.frame_id = id;  // (sic: the marker id, common.hpp:73)
            ps.header.sec = header.sec;
            ps.header.nsec = header.nsec;
            ps.pose = pose;
            out->markers.push_back(ps);
            Detection2D det;
            det.header = header;
            ObjectHypothesisWithPose hyp;
            hyp.id = markers[i].id;
            hyp.pose = pose;
            if (pcov && pcov->status == 0) std::copy(pcov->cov_pose, pcov->cov_pose + 36, hyp.covariance.begin());
            det.results.push_back(hyp);
            out->array.detections.push_back(det);
        }
        for (const fid_stag_bundle_pose_out &bp : bposes) {
            if (params.layout_standalone[(size_t)bp.bundle]) continue;
            const Pose pose = poseOf(bp.R, bp.tvec);
            const std::string &frame = params.layout_frames[(size_t)bp.bundle];
            if (params.publish_tf) {
                TransformStamped t;
                t.header = header;
                t.child_frame_id = params.tag_tf_prefix + frame;
                t.tx = pose.px; t.ty = pose.py; t.tz = pose.pz;
                t.qx = pose.ox; t.qy = pose.oy; t.qz = pose.oz; t.qw = pose.ow;
                out->tf.push_back(t);
            }
            PoseStamped ps;
            ps.header.frame_id = frame;
            ps.header.sec = header.sec;
            ps.header.nsec = header.nsec;
            ps.pose = pose;
            out->bundles.push_back(ps);
        }
        out->array_published = true;
    }

    Stag stag;
    std::vector<uint8_t> gray_;
    int maxW = 0, maxH = 0, dev = 0;
    fid_jpeg_ctx *jctx = nullptr;  // made when the first compressed JPEG frame arrives
    fid_jpeg_enc_ctx *ectx = nullptr;  // made when the first compressed marker image is asked for
    std::string last_error;
};

}  // namespace fiducials_amd
#endif
