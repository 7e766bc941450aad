// diamond_detector.hpp -- the host side of the diamond entry points (include/fid_abi.h: "ChArUco diamonds"): the diamonds among the markers
// of the last detect call or of markers and an image from host memory, and their poses as fiducials of side square_len
// (cv::aruco::detectCharucoDiamond, then estimatePoseSingleMarkers on the diamond corners).  Header only; needs nothing but the C-ABI.
#pragma once

#include <cstdint>
#include <vector>

#include "fid_abi.h"

namespace fiducials_amd {

class DiamondDetector {
public:
    // ctx: an aruco context; it is borrowed, not owned.  square_marker_rate = square_len / marker_len of the print.
    DiamondDetector(fid_ctx *ctx, double square_marker_rate) : ctx_(ctx)
    {
        fid_default_diamond_opts(&opts_);
        opts_.square_marker_rate = square_marker_rate;
    }

    fid_diamond_opts &options() { return opts_; }

    // the diamonds of every frame of the last fid_detect* / fid_collect: per_frame[f] = frame f's, in the order of their first markers
    fid_status detectLast(int frames, std::vector<std::vector<fid_diamond>> *per_frame) const
    {
        const int cap = FID_DIAMOND_MAX_PER_FRAME;
        std::vector<fid_diamond> flat((size_t)(frames > 0 ? frames : 1) * cap);
        std::vector<int32_t> n((size_t)(frames > 0 ? frames : 1), 0);
        const fid_status rc = fid_diamonds_last(ctx_, &opts_, flat.data(), cap, n.data());
        if (rc != FID_OK) return rc;
        per_frame->assign((size_t)frames, {});
        for (int f = 0; f < frames; f++) (*per_frame)[(size_t)f].assign(flat.begin() + (long)f * cap, flat.begin() + (long)f * cap + n[(size_t)f]);
        return rc;
    }

    // the same on markers and a mono8 image from host memory
    fid_status detect(const std::vector<fid_marker> &markers, const uint8_t *img, int width, int height, int stride, std::vector<fid_diamond> *out) const
    {
        out->assign((size_t)FID_DIAMOND_MAX_PER_FRAME, fid_diamond{});
        int32_t n = 0;
        const fid_status rc = fid_diamonds_detect(ctx_, &opts_, markers.empty() ? nullptr : markers.data(), (int32_t)markers.size(), img, width, height,
                                                  stride, out->data(), (int32_t)out->size(), &n);
        out->resize(rc == FID_OK ? (size_t)n : 0);
        return rc;
    }

    // every diamond as a fiducial of side square_len centred on its middle square
    fid_status pose(const fid_camera &cam, const std::vector<fid_diamond> &diamonds, double square_len, std::vector<fid_pose_out> *out) const
    {
        out->assign(diamonds.size(), fid_pose_out{});
        return fid_diamond_pose_cam(ctx_, &cam, diamonds.empty() ? nullptr : diamonds.data(), (int32_t)diamonds.size(), square_len, out->data());
    }

private:
    fid_ctx *ctx_;
    fid_diamond_opts opts_;
};

}  // namespace fiducials_amd
