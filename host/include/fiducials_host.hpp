// fiducials_host.hpp -- the host side of the aruco_detect drop-in in the reference's own language: a ROS-free FiducialsNode
// with the callbacks, members and parameter names of aruco_detect/src/aruco_detect.cpp:88-147, on top of the C-ABI
// (include/fid_abi.h).  No ROS, catkin or OpenCV exists in this image, so the message types are plain structs with the fields
// of the .msg files and "publishing" is returning the message; everything else -- gating, latching of the first CameraInfo,
// ignore list, per-id lengths, header rules, quaternion -- is the node's logic, so that the node proper is this class plus
// ros::Subscriber / Publisher glue.  The arithmetic of the hot path is NOT here: it is behind fid_detect / fid_pose_last.
#ifndef FIDUCIALS_HOST_HPP
#define FIDUCIALS_HOST_HPP
#include <array>
#include <cstdint>
#include <map>
#include <cstddef>
#include <string>
#include <vector>

#include "fid_abi.h"

namespace fiducials_amd {

struct Header {  // std_msgs/Header
    uint32_t seq = 0;
    uint32_t sec = 0, nsec = 0;
    std::string frame_id;
};
struct Image {  // sensor_msgs/Image
    Header header;
    uint32_t height = 0, width = 0;
    std::string encoding;  // "mono8", "bgr8", "rgb8", "bgra8", "rgba8"; "mono16", "bgr16", "rgb16", "bgra16", "rgba16", "bayer_{rggb,bggr,gbrg,grbg}8"
    uint8_t is_bigendian = 0;
    uint32_t step = 0;
    std::vector<uint8_t> data;
};
struct CompressedImage {  // sensor_msgs/CompressedImage: what arrives with image_transport's `compressed` (the launch default)
    Header header;
    std::string format;  // "jpeg", "bgr8; jpeg compressed bgr8" or "mono8; png compressed " as compressed_image_transport writes it
                         // (the data decides: JPEG goes to the device decoder, PNG through fid_png_decode on the host)
    std::vector<uint8_t> data;
};
struct CameraInfo {  // sensor_msgs/CameraInfo (the fields the node reads)
    Header header;
    uint32_t height = 0, width = 0;
    std::string distortion_model;
    std::vector<double> D;
    std::array<double, 9> K{};
};
struct Fiducial {  // fiducial_msgs/Fiducial
    int32_t fiducial_id = 0, direction = 0;
    double x0 = 0, y0 = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0, x3 = 0, y3 = 0;
};
struct FiducialArray {
    Header header;
    int32_t image_seq = 0;
    std::vector<Fiducial> fiducials;
};
struct FiducialTransform {  // fiducial_msgs/FiducialTransform
    int32_t fiducial_id = 0;
    double tx = 0, ty = 0, tz = 0;          // geometry_msgs/Transform.translation
    double qx = 0, qy = 0, qz = 0, qw = 1;  // geometry_msgs/Transform.rotation
    double image_error = 0, object_error = 0, fiducial_area = 0;
};
struct FiducialTransformArray {
    Header header;
    int32_t image_seq = 0;
    std::vector<FiducialTransform> transforms;
};

// ---- the other output surface of poseEstimateCallback (aruco_detect.cpp:462-478, 501-524): vision_msgs and tf2
struct Pose {  // geometry_msgs/Pose
    double px = 0, py = 0, pz = 0;
    double ox = 0, oy = 0, oz = 0, ow = 1;
};
struct PoseStamped {  // geometry_msgs/PoseStamped
    Header header;
    Pose pose;
};
struct ObjectHypothesisWithPose {  // vision_msgs/ObjectHypothesisWithPose (Noetic: int64 id, float64 score, PoseWithCovariance)
    int64_t id = 0;
    double score = 0;
    Pose pose;
    std::array<double, 36> covariance{};
};
struct PoseWithCovarianceStamped {  // geometry_msgs/PoseWithCovarianceStamped
    Header header;
    Pose pose;
    std::array<double, 36> covariance{};  // x, y, z, rotation about X, Y, Z (of the parent frame), row-major
};
struct Detection2D {  // vision_msgs/Detection2D: the node fills `results` only (header, bbox and source_img stay default)
    Header header;
    std::vector<ObjectHypothesisWithPose> results;
};
struct Detection2DArray {
    Header header;
    std::vector<Detection2D> detections;
};
struct TransformStamped {  // geometry_msgs/TransformStamped, what tf2_ros::TransformBroadcaster::sendTransform is handed
    Header header;
    std::string child_frame_id;
    double tx = 0, ty = 0, tz = 0;
    double qx = 0, qy = 0, qz = 0, qw = 1;
};
// everything one poseEstimateCallback publishes: `~vis_msgs` selects which of the two arrays goes to fiducial_transforms
// (:666-669, 534-537), `~publish_fiducial_tf` whether `tf` is broadcast (:501-524)
struct PoseOutputs {
    bool vis_msgs = false;
    FiducialTransformArray fta;
    Detection2DArray vma;
    std::vector<TransformStamped> tf;
    // with ~map_file set and at least one mapped fiducial in sight: the camera in the map (frame_id "map"), one solvePnP over the
    // corners of every mapped marker (fid_map_pose_last); empty otherwise
    std::vector<PoseStamped> map_pose;
    // with ~pose_covariance set: the same pose with cov_cam_pose of fid_map_pose_last_cov_cam (frame_id "map"), beside map_pose,
    // which stays what it is; empty otherwise
    std::vector<PoseWithCovarianceStamped> map_pose_cov;
    // with ~map_outlier_px > 0: the fiducial ids that the consensus map pose left out (fid_map_robust_out's outlier_mask read against
    // the used markers), in list order; on no consensus every used id.  Empty otherwise
    std::vector<int32_t> map_outliers;
};

// ROS 1 wire format of the two output messages (little-endian, packed)
std::vector<uint8_t> serialize(const FiducialArray &m);
std::vector<uint8_t> serialize(const FiducialTransformArray &m);
bool deserialize(const std::vector<uint8_t> &b, FiducialTransformArray *m);

// aruco::getPredefinedDictionary(dicno) (aruco_detect.cpp:671): tables from <data_dir>/dict_*.txt (provenance:
// tools/make_dictionaries.py); the returned object owns the byte list fid_dict points into
struct Dictionary {
    int markerSize = 0, maxCorrectionBits = 0, nMarkers = 0;
    std::vector<uint8_t> bytesList;  // nMarkers x 4 rotations x nbytes
    fid_dict view() const;
};
Dictionary getPredefinedDictionary(int dicno, const std::string &data_dir);
// ... from a table file the deployer has (fid_dict_load_file: OpenCV's predefined_dictionaries.hpp as text, a FileStorage
// YAML, or a dict_*.txt): every enum value 0..16, or -1 for a custom dictionary whose sizes the YAML states
Dictionary loadDictionaryFile(int dicno, const std::string &table_file);

class FiducialsNode {
   public:
    struct Params {  // the private parameters of the node with their defaults (aruco_detect.cpp:609-627) ...
        bool publish_images = false;
        double fiducial_len = 0.14;
        int dictionary = 7;
        bool do_pose_estimation = true;
        bool publish_fiducial_tf = true;
        bool vis_msgs = false;
        bool verbose = false;
        std::string ignore_fiducials;
        std::string fiducial_len_override;
        fid_params detector;  // ... and the detector parameters as the node sets them (:690-727)
        std::string data_dir = "fiducials_amd/data";
        std::string dictionary_file;  // non-empty: the table of ~dictionary comes from this file (loadDictionaryFile) -- the way to
                                      // run the families whose shipped tables are fillers (4X4_1000, 6X6, 7X7, ARUCO_ORIGINAL)
        std::string map_file;  // non-empty: a fiducial_slam map file (fid_map_load_file; ~fiducial_len and ~fiducial_len_override give
                               // the lengths); poseEstimateCallback then also reports the camera in the map (PoseOutputs::map_pose)
        // fill ObjectHypothesisWithPose::covariance with the pose's covariance (fid_abi.h, "pose covariance": cov_pose; 36 zeros for
        // a record whose status is not 0) and report PoseOutputs::map_pose_cov; off: every output is what it was
        bool pose_covariance = false;
        double pose_covariance_sigma_px = 1.0;  // the corner noise in pixels; 0: the a-posteriori estimate from the residuals
        // > 0: map_pose is the consensus pose (fid_abi.h, "map pose that survives wrong markers": fid_map_pose_robust_last_cam with
        // this inlier_px -- the header recommends 4.0 -- and map_min_markers), empty on no consensus; the ids left out go to
        // PoseOutputs::map_outliers, and map_pose_cov comes from fid_map_pose_cov_cam on the inliers.  0: off, every output is
        // byte for byte what it was
        double map_outlier_px = 0.0;
        int map_min_markers = 2;
        int device = 0, max_width = 1920, max_height = 1080;
        Params();
    };
    explicit FiducialsNode(const Params &p);  // throws std::runtime_error without a device: there is no CPU path
    ~FiducialsNode();
    FiducialsNode(const FiducialsNode &) = delete;
    FiducialsNode &operator=(const FiducialsNode &) = delete;

    // the callbacks (same names as the reference).  The two image-path callbacks return true when the node would have
    // published, the message is then in *out
    void configCallback(const fid_params &config, uint32_t level);  // :257-298
    void ignoreCallback(const std::string &msg);                     // :300-305
    void camInfoCallback(const CameraInfo &msg);                     // :307-330
    bool imageCallback(const Image &msg, FiducialArray *out);        // :332-395
    // ... and what image_pub publishes on /fiducial_images when ~publish_images is set (:381-387): the BGR8 copy of the frame
    // with aruco::drawDetectedMarkers' marker outlines on it (fid_draw_detected_markers: the exactly restated part of the
    // overlay; include/fid_abi.h lists what is not drawn).  *image is filled only when publish_images is set (returns the same
    // as the two-argument form).
    bool imageCallback(const Image &msg, FiducialArray *out, Image *image);
    // the same callback for a frame that arrives compressed (aruco_detect.launch:6 transport=compressed): the JPEG is decoded
    // on the device (fid_jpeg_decode: what the subscriber plugin's cv::imdecode + toCvCopy(BGR8) + BGR2GRAY produce) and the
    // detector runs on the device-resident gray image
    bool compressedImageCallback(const CompressedImage &msg, FiducialArray *out);
    // ... and with the image /fiducial_images carries when ~publish_images is set: the decoded BGR8 frame with the marker outlines
    // (drawn only when markers were found, :381), as imageCallback(msg, out, image) makes it for a raw frame.  A JPEG is then
    // decoded to BGR8 on the device, detected there and drawn there (fid_jpeg_marker_image); a PNG is decoded to BGR8 and drawn on
    // the host.  The vertices are those of the two-argument form.  image->data is empty unless an image is published; with
    // publish_images off or image == nullptr the call is the two-argument form.
    bool compressedImageCallback(const CompressedImage &msg, FiducialArray *out, Image *image);
    // ... and with what /fiducial_images/compressed carries (image_transport offers that topic for every image publisher,
    // aruco_detect.cpp:662): the same marker image as the JPEG file compressed_image_transport's publisher makes of it
    // (cv::imencode(".jpg") at its default quality), format "bgr8; jpeg compressed bgr8".  For a JPEG frame the image is drawn AND
    // compressed on the device (fid_jpeg_marker_jpeg): only the file crosses to the host.  A PNG frame's image is drawn on the host
    // and compressed on the device (fid_jpeg_encode).  image->data is empty unless an image is published.
    bool compressedImageCallback(const CompressedImage &msg, FiducialArray *out, CompressedImage *image);
    bool compressedImageCallback(const CompressedImage &msg, FiducialArray *out, std::nullptr_t) { return compressedImageCallback(msg, out, (Image *)nullptr); }
    bool poseEstimateCallback(const FiducialArray &msg, FiducialTransformArray *out);  // :397-538 (fiducial_msgs view)
    bool poseEstimateCallback(const FiducialArray &msg, PoseOutputs *out);             // ... everything it publishes
    bool enableDetectionsCallback(bool data, std::string *message);  // :573-588

    // state the reference keeps as members (read-only views for tests)
    const std::vector<int> &getIds() const { return ids; }
    const std::vector<int> &getIgnoreIds() const { return ignoreIds; }
    const std::map<int, double> &getFiducialLens() const { return fiducialLens; }
    bool haveCameraInfo() const { return haveCamInfo; }
    const std::string &lastError() const { return last_error; }

   private:
    void handleIgnoreString(const std::string &str);           // :540-571
    void handleLenOverrideString(const std::string &str);      // :627-660
    bool publishVertices(const Header &h, int32_t n, FiducialArray *out);  // the tail of imageCallback (:342-379)
    fid_ctx *ctx = nullptr;
    bool compressedFrame(const CompressedImage &msg, FiducialArray *out, Image *image, CompressedImage *cimage);
    bool publishCompressed(const Header &h, const uint8_t *raw, int32_t w, int32_t ht, int32_t n, CompressedImage *cimage);
    fid_jpeg_ctx *jctx = nullptr;  // made when the first compressed frame arrives
    fid_jpeg_enc_ctx *ectx = nullptr;  // made when the first compressed marker image is asked for
    std::vector<uint8_t> png_frame;  // a PNG frame decoded on the host (fid_png_decode), reused from frame to frame
    std::vector<uint8_t> converted;  // (round 5: the BGR8 copy of a 16-bit / Bayer frame made before the detection; unused since ABI 7)
    bool raw_encoding = false;       // the last frame came in a raw-camera encoding (Bayer / 16 bit / UYVY): detected on the message bytes
    int maxW = 0, maxH = 0, dev = 0;
    Dictionary dict;
    fid_params detectorParams;
    std::vector<fid_marker> markers;   // corners / ids of the last image (the reference's `corners`, `ids` members, :101-102)
    std::vector<int> ids;
    std::vector<int> ignoreIds;
    std::map<int, double> fiducialLens;
    fid_camera camera = {};     // CameraInfo as the library takes it: the distortion model with its coefficients
    std::string camInfoError;   // why the last CameraInfo was refused (a distortion model the library does not pose under)
    bool haveCamInfo = false, enable_detections = true, doPoseEstimation = true, verbose = false;
    bool vis_msgs = false, publishFiducialTf = true, publish_images = false;
    bool haveMap = false;
    std::vector<int> mapIds;  // the ids the map names, ascending (the used markers of a frame are recounted against it)
    double mapOutlierPx = 0.0;
    int mapMinMarkers = 2;
    bool poseCovariance = false;
    double poseCovarianceSigmaPx = 1.0;
    double fiducial_len = 0.14;
    int frameNum = 0;
    std::string frameId, last_error;
};

}  // namespace fiducials_amd
#endif
