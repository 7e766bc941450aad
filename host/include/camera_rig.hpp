// camera_rig.hpp -- the host side of the rig entry points (include/fid_abi.h: "one rig pose per time step from all cameras of a
// multi-camera rig"): the cameras of a body as CameraInfo says them and as a static transform places them, and one pose of that body
// in the map per time step of the last detect call, in geometry_msgs/PoseWithCovarianceStamped's shape with the per-camera
// reprojection errors beside it.  Header only above fiducials_host.hpp's message structs; needs nothing else but the C-ABI.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "fid_abi.h"
#include "fiducials_host.hpp"

namespace fiducials_amd {

// one time step's result: the rig ("child_frame_id") in the map (header.frame_id)
struct RigPose {
    PoseWithCovarianceStamped pose;  // covariance: cov_cam_pose of the joint solve, zero without sigma_px or where its status is not 0
    std::string child_frame_id;
    bool valid = false;              // false: nobody saw the map in this time step
    fid_rig_pose_out record{};
    std::vector<double> err_per_camera;  // px^2, one per camera of the rig (0 for a camera without a used marker)
};

class CameraRig {
public:
    explicit CameraRig(std::string rig_frame = "base_link") : rig_frame_(std::move(rig_frame)) {}

    // a camera of the rig: its CameraInfo (K, D, distortion_model) and its pose in the rig frame, a static transform's translation
    // and quaternion (x, y, z, w).  The order of the calls is the order of the frames within a time step.
    fid_status addCamera(const CameraInfo &info, const double xyz[3], const double quat_xyzw[4])
    {
        fid_camera cam = {};
        fid_status rc = fid_camera_from_info(info.distortion_model.c_str(), info.K.data(), info.D.data(), (int32_t)info.D.size(), &cam);
        if (rc != FID_OK) {
            last_error_ = fid_camera_last_error();
            return rc;
        }
        fid_rig_camera rcam;
        rc = fid_rig_camera_from_tf(xyz, quat_xyzw, &cam, &rcam);
        if (rc != FID_OK) {
            last_error_ = "the camera's transform must be finite and its quaternion not zero";
            return rc;
        }
        cams_.push_back(rcam);
        return FID_OK;
    }

    size_t size() const { return cams_.size(); }
    const std::vector<fid_rig_camera> &cameras() const { return cams_; }
    const std::string &lastError() const { return last_error_; }

    // hand the rig to a context (fid_set_rig)
    fid_status apply(fid_ctx *ctx)
    {
        const fid_status rc = fid_set_rig(ctx, cams_.empty() ? nullptr : cams_.data(), (int32_t)cams_.size());
        if (rc != FID_OK) last_error_ = fid_last_error(ctx);
        return rc;
    }

    // one result per time step of the context's last detect call, whose frames are camera f % C of step f / C under the rig the
    // context holds (apply): the context says how many time steps that is (fid_rig_steps_last).  sigma_px < 0: no covariance
    fid_status pose(fid_ctx *ctx, const Header &stamp, std::vector<RigPose> *out, double sigma_px = -1.)
    {
        const int C = (int)cams_.size();
        int32_t steps = 0;
        const fid_status rcs = fid_rig_steps_last(ctx, &steps);
        if (rcs != FID_OK) {
            last_error_ = fid_last_error(ctx);
            return rcs;
        }
        std::vector<fid_rig_pose_out> rec((size_t)steps);
        std::vector<fid_map_pose_cov> cov(sigma_px >= 0. ? rec.size() : 0);
        const fid_status rc = fid_rig_pose_last(ctx, rec.data(), (int32_t)rec.size(), sigma_px >= 0. ? sigma_px : 0., cov.empty() ? nullptr : cov.data());
        if (rc != FID_OK) {
            last_error_ = fid_last_error(ctx);
            return rc;
        }
        out->assign((size_t)steps, RigPose{});
        for (int s = 0; s < steps; s++) {
            RigPose &p = (*out)[(size_t)s];
            p.record = rec[(size_t)s];
            p.valid = p.record.n_markers > 0;
            p.child_frame_id = rig_frame_;
            p.pose.header = stamp;
            p.pose.header.frame_id = "map";
            p.err_per_camera.assign(p.record.err_per_camera, p.record.err_per_camera + C);
            if (!p.valid) continue;
            double q[4];
            quaternion(p.record.rig_R, q);
            p.pose.pose.px = p.record.rig_t[0]; p.pose.pose.py = p.record.rig_t[1]; p.pose.pose.pz = p.record.rig_t[2];
            p.pose.pose.ox = q[0]; p.pose.pose.oy = q[1]; p.pose.pose.oz = q[2]; p.pose.pose.ow = q[3];
            if (!cov.empty() && cov[(size_t)s].pose.status == 0)
                for (int i = 0; i < 36; i++) p.pose.covariance[(size_t)i] = cov[(size_t)s].cov_cam_pose[i];
        }
        return FID_OK;
    }

private:
    // a row-major rotation as a unit quaternion x y z w (tf2::Matrix3x3::getRotation's branches)
    static void quaternion(const double R[9], double q[4])
    {
        const double tr = R[0] + R[4] + R[8];
        if (tr > 0) {
            const double s4 = 2.0 * std::sqrt(tr + 1.0);
            q[3] = 0.25 * s4; q[0] = (R[7] - R[5]) / s4; q[1] = (R[2] - R[6]) / s4; q[2] = (R[3] - R[1]) / s4;
        } else if (R[0] > R[4] && R[0] > R[8]) {
            const double s4 = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]);
            q[3] = (R[7] - R[5]) / s4; q[0] = 0.25 * s4; q[1] = (R[1] + R[3]) / s4; q[2] = (R[2] + R[6]) / s4;
        } else if (R[4] > R[8]) {
            const double s4 = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]);
            q[3] = (R[2] - R[6]) / s4; q[0] = (R[1] + R[3]) / s4; q[1] = 0.25 * s4; q[2] = (R[5] + R[7]) / s4;
        } else {
            const double s4 = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]);
            q[3] = (R[3] - R[1]) / s4; q[0] = (R[2] + R[6]) / s4; q[1] = (R[5] + R[7]) / s4; q[2] = 0.25 * s4;
        }
    }

    std::string rig_frame_, last_error_;
    std::vector<fid_rig_camera> cams_;
};

}  // namespace fiducials_amd
