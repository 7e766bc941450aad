// camera_calibrator.hpp -- the host side of fid_calibrate_map (include/fid_abi.h: "camera calibration from views of the map"):
// collect the markers of frames that show the context's map, calibrate, and hand the result on as sensor_msgs/CameraInfo's fields
// or as the YAML file camera drivers load through `camera_info_url` (camera_calibration_parsers' layout).  CharucoCalibrator is the
// same over fid_calibrate_charuco: the views are the chessboard corner records of frames that show the context's ChArUco board.
// Header only; needs nothing but the C-ABI.
#pragma once

#include <array>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fid_abi.h"

namespace fiducials_amd {

// the fields of sensor_msgs/CameraInfo a calibration fills
struct CalibratedCameraInfo {
    uint32_t width = 0, height = 0;
    std::string distortion_model;
    std::vector<double> D;
    std::array<double, 9> K{};
    std::array<double, 9> R{};   // identity: one camera, no rectification
    std::array<double, 12> P{};  // [K | 0]
};

class CameraCalibrator {
public:
    // ctx: a context with its map set (fid_set_map); it is borrowed, not owned
    CameraCalibrator(fid_ctx *ctx, int image_width, int image_height) : ctx_(ctx), w_(image_width), h_(image_height) {}

    // the markers of one frame (fid_detect's output); a frame without markers may be added, it is skipped by the solve
    void addView(const fid_marker *markers, int n)
    {
        views_.emplace_back(markers, markers + (n > 0 ? n : 0));
    }
    size_t size() const { return views_.size(); }
    void clear() { views_.clear(); }

    // fid_calibrate_map over the views added so far.  *cam_io: model, n_dist, start / fixed values in, the calibrated camera out.
    fid_status calibrate(const fid_calib_opts &opts, fid_camera *cam_io, fid_calib_out *out, std::vector<fid_calib_view> *views = nullptr) const
    {
        size_t cap = 1;
        for (const auto &v : views_) cap = v.size() > cap ? v.size() : cap;
        std::vector<fid_marker> packed(views_.size() * cap);
        std::vector<int32_t> n(views_.size());
        for (size_t i = 0; i < views_.size(); i++) {
            n[i] = (int32_t)views_[i].size();
            for (size_t k = 0; k < views_[i].size(); k++) packed[i * cap + k] = views_[i][k];
        }
        std::vector<fid_calib_view> vout(views_.size());
        const fid_status rc = fid_calibrate_map(ctx_, packed.data(), n.data(), (int32_t)views_.size(), (int32_t)cap, w_, h_, &opts, cam_io, out,
                                                vout.empty() ? nullptr : vout.data());
        if (rc == FID_OK && views) *views = vout;
        return rc;
    }

    // fid_camera -> CameraInfo's fields: distortion model string, K, D, R = I, P = [K | 0]
    static bool toCameraInfo(const fid_camera &cam, int width, int height, CalibratedCameraInfo *info)
    {
        char name[32];
        double D[12];
        int32_t n_D = 0;
        if (!info || fid_camera_to_info(&cam, name, info->K.data(), D, &n_D) != FID_OK) return false;
        info->width = (uint32_t)width;
        info->height = (uint32_t)height;
        info->distortion_model = name;
        info->D.assign(D, D + n_D);
        info->R = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) info->P[4 * r + c] = info->K[3 * r + c];
            info->P[4 * r + 3] = 0.;
        }
        return true;
    }

    // the file camera drivers load through camera_info_url: image_width, image_height, camera_name, camera_matrix, distortion_model,
    // distortion_coefficients, rectification_matrix, projection_matrix, each matrix with rows, cols, data.  %.17g: the doubles come
    // back bit for bit.
    static bool writeYaml(const std::string &path, const std::string &camera_name, const CalibratedCameraInfo &info)
    {
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) return false;
        std::fprintf(f, "image_width: %u\nimage_height: %u\ncamera_name: %s\n", info.width, info.height, camera_name.c_str());
        matrix(f, "camera_matrix", 3, 3, info.K.data());
        std::fprintf(f, "distortion_model: %s\n", info.distortion_model.c_str());
        matrix(f, "distortion_coefficients", 1, (int)info.D.size(), info.D.data());
        matrix(f, "rectification_matrix", 3, 3, info.R.data());
        matrix(f, "projection_matrix", 3, 4, info.P.data());
        return std::fclose(f) == 0;
    }

private:
    static void matrix(FILE *f, const char *name, int rows, int cols, const double *data)
    {
        std::fprintf(f, "%s:\n  rows: %d\n  cols: %d\n  data: [", name, rows, cols);
        for (int i = 0; i < rows * cols; i++) std::fprintf(f, "%s%.17g", i ? ", " : "", data[i]);
        std::fprintf(f, "]\n");
    }

    fid_ctx *ctx_;
    int w_, h_;
    std::vector<std::vector<fid_marker>> views_;
};

// fid_calibrate_charuco (include/fid_abi.h: "camera calibration from ChArUco corners") over views collected one by one; the result goes
// on through CameraCalibrator::toCameraInfo / writeYaml
class CharucoCalibrator {
public:
    // ctx: a context with its board set (fid_set_charuco_board); it is borrowed, not owned
    CharucoCalibrator(fid_ctx *ctx, int image_width, int image_height) : ctx_(ctx), w_(image_width), h_(image_height) {}

    // the corner records of one frame (fid_charuco_last_cam's or fid_charuco_interpolate_cam's output); a frame without corners may be
    // added, it is skipped by the solve
    void addView(const fid_charuco_corner *corners, int n)
    {
        views_.emplace_back(corners, corners + (n > 0 ? n : 0));
    }
    size_t size() const { return views_.size(); }
    void clear() { views_.clear(); }

    // fid_calibrate_charuco over the views added so far.  *cam_io: model, n_dist, start / fixed values in, the calibrated camera out.
    fid_status calibrate(const fid_calib_opts &opts, fid_camera *cam_io, fid_calib_out *out, std::vector<fid_calib_view> *views = nullptr) const
    {
        size_t cap = 1;
        for (const auto &v : views_) cap = v.size() > cap ? v.size() : cap;
        std::vector<fid_charuco_corner> packed(views_.size() * cap);
        std::vector<int32_t> n(views_.size());
        for (size_t i = 0; i < views_.size(); i++) {
            n[i] = (int32_t)views_[i].size();
            for (size_t k = 0; k < views_[i].size(); k++) packed[i * cap + k] = views_[i][k];
        }
        std::vector<fid_calib_view> vout(views_.size());
        const fid_status rc = fid_calibrate_charuco(ctx_, packed.data(), n.data(), (int32_t)views_.size(), (int32_t)cap, w_, h_, &opts, cam_io, out,
                                                    vout.empty() ? nullptr : vout.data());
        if (rc == FID_OK && views) *views = vout;
        return rc;
    }

private:
    fid_ctx *ctx_;
    int w_, h_;
    std::vector<std::vector<fid_charuco_corner>> views_;
};

}  // namespace fiducials_amd
