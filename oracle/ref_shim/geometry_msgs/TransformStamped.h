// Functional stand-in (TEST INFRASTRUCTURE): our own text, just enough of the third-party names for the reference's
// GroundSegmentation translation unit to compile unmodified and run (oracle/ref_build.py).  It is not the library it is named after,
// builds no other part of the reference and pins no third-party arithmetic (tools/pin/ does that).
// geometry_msgs/TransformStamped.h and PointStamped: plain structs with the message fields, zero-initialised as ROS messages are.
#pragma once

#include <ros/ros.h>

#include <string>

namespace std_msgs {
struct Header {
    unsigned int seq = 0;
    ros::Time stamp;
    std::string frame_id;
};
} // namespace std_msgs

namespace geometry_msgs {
struct Vector3 {
    double x = 0.0, y = 0.0, z = 0.0;
};
struct Point {
    double x = 0.0, y = 0.0, z = 0.0;
};
struct Quaternion {
    double x = 0.0, y = 0.0, z = 0.0, w = 0.0;
};
struct Transform {
    Vector3 translation;
    Quaternion rotation;
};
struct TransformStamped {
    std_msgs::Header header;
    std::string child_frame_id;
    Transform transform;
};
struct PointStamped {
    std_msgs::Header header;
    Point point;
};
} // namespace geometry_msgs
