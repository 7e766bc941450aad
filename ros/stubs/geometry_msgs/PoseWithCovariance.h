#ifndef GEOMETRY_MSGS_POSEWITHCOVARIANCE_STUB_H
#define GEOMETRY_MSGS_POSEWITHCOVARIANCE_STUB_H
#include <geometry_msgs/Transform.h>
#include <array>
namespace geometry_msgs {
struct PoseWithCovariance {  // geometry_msgs/PoseWithCovariance.msg
    Pose pose;
    std::array<double, 36> covariance{};
};
}  // namespace geometry_msgs
#endif
