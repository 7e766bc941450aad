#ifndef GEOMETRY_MSGS_POSEWITHCOVARIANCESTAMPED_STUB_H
#define GEOMETRY_MSGS_POSEWITHCOVARIANCESTAMPED_STUB_H
#include <geometry_msgs/PoseWithCovariance.h>
#include <std_msgs/Header.h>
namespace geometry_msgs {
struct PoseWithCovarianceStamped {  // geometry_msgs/PoseWithCovarianceStamped.msg
    std_msgs::Header header;
    PoseWithCovariance pose;
};
}  // namespace geometry_msgs
#endif
