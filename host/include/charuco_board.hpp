// charuco_board.hpp -- the host side of the ChArUco entry points (include/fid_abi.h: "ChArUco boards"): a board on an aruco context, the
// chessboard corners of the last detect call or of markers and an image from host memory, and the board pose over them
// (cv::aruco::interpolateCornersCharuco / estimatePoseCharucoBoard).  Header only; needs nothing but the C-ABI.
#pragma once

#include <cstdint>
#include <vector>

#include "fid_abi.h"

namespace fiducials_amd {

class CharucoBoard {
public:
    // ctx: an aruco context; it is borrowed, not owned.  The board is set on it by create() and cleared by the destructor.
    explicit CharucoBoard(fid_ctx *ctx) : ctx_(ctx) {}
    ~CharucoBoard()
    {
        if (set_) (void)fid_set_charuco_board(ctx_, nullptr);
    }
    CharucoBoard(const CharucoBoard &) = delete;
    CharucoBoard &operator=(const CharucoBoard &) = delete;

    // cv::aruco::CharucoBoard::create: squares_x x squares_y squares, the markers first_id, first_id + 1, ... of the context's dictionary
    fid_status create(int squares_x, int squares_y, double square_len, double marker_len, int first_id = 0)
    {
        const fid_charuco_board b = {squares_x, squares_y, square_len, marker_len, first_id, 0};
        const fid_status rc = fid_set_charuco_board(ctx_, &b);
        if (rc == FID_OK) {
            board_ = b;
            set_ = true;
        }
        return rc;
    }
    int corners() const { return set_ ? (board_.squares_x - 1) * (board_.squares_y - 1) : 0; }
    int markers() const { return set_ ? board_.squares_x * board_.squares_y / 2 : 0; }
    // the object point of chessboard corner id (the header's: rounded through float)
    void objectPoint(int id, double xyz[3]) const
    {
        const int row = board_.squares_x - 1;
        xyz[0] = (double)(float)((id % row + 1) * board_.square_len);
        xyz[1] = (double)(float)((id / row + 1) * board_.square_len);
        xyz[2] = 0.;
    }

    // the corners of every frame of the last fid_detect* / fid_collect: per_frame[f] = frame f's, ascending id.  cam may be NULL
    // (positions from the per-marker homographies).
    fid_status interpolateLast(const fid_camera *cam, int frames, std::vector<std::vector<fid_charuco_corner>> *per_frame, int min_markers = 2) const
    {
        const int cap = corners() > 0 ? corners() : 1;
        std::vector<fid_charuco_corner> flat((size_t)(frames > 0 ? frames : 1) * cap);
        std::vector<int32_t> n((size_t)(frames > 0 ? frames : 1), 0);
        const fid_status rc = fid_charuco_last_cam(ctx_, cam, min_markers, flat.data(), cap, n.data());
        if (rc != FID_OK) return rc;
        per_frame->assign((size_t)frames, {});
        for (int f = 0; f < frames; f++) (*per_frame)[(size_t)f].assign(flat.begin() + (long)f * cap, flat.begin() + (long)f * cap + n[(size_t)f]);
        return rc;
    }

    // the same on markers and a mono8 image from host memory
    fid_status interpolate(const fid_camera *cam, const std::vector<fid_marker> &markers, const uint8_t *img, int width, int height, int stride,
                           std::vector<fid_charuco_corner> *out, int min_markers = 2) const
    {
        out->assign((size_t)(corners() > 0 ? corners() : 1), fid_charuco_corner{});
        int32_t n = 0;
        const fid_status rc = fid_charuco_interpolate_cam(ctx_, cam, markers.empty() ? nullptr : markers.data(), (int32_t)markers.size(), img, width, height,
                                                          stride, min_markers, out->data(), (int32_t)out->size(), &n);
        out->resize(rc == FID_OK ? (size_t)n : 0);
        return rc;
    }

    // estimatePoseCharucoBoard over the frames of the last call (one record per frame) ...
    fid_status poseLast(const fid_camera &cam, int frames, std::vector<fid_charuco_pose_out> *out, int min_markers = 2) const
    {
        out->assign((size_t)(frames > 0 ? frames : 1), fid_charuco_pose_out{});
        const fid_status rc = fid_charuco_pose_last_cam(ctx_, &cam, min_markers, out->data(), (int32_t)out->size());
        out->resize(rc == FID_OK && frames > 0 ? (size_t)frames : 0);
        return rc;
    }
    // ... and over corners the caller holds (their refined x, y)
    fid_status pose(const fid_camera &cam, const std::vector<fid_charuco_corner> &corners, fid_charuco_pose_out *out) const
    {
        std::vector<float> xy(2 * corners.size());
        std::vector<int32_t> ids(corners.size());
        for (size_t i = 0; i < corners.size(); i++) {
            xy[2 * i] = corners[i].x;
            xy[2 * i + 1] = corners[i].y;
            ids[i] = corners[i].id;
        }
        return fid_charuco_pose_cam(ctx_, &cam, xy.data(), ids.data(), (int32_t)corners.size(), out);
    }

private:
    fid_ctx *ctx_;
    fid_charuco_board board_ = {};
    bool set_ = false;
};

}  // namespace fiducials_amd
