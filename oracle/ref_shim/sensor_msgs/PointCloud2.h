// Functional stand-in (TEST INFRASTRUCTURE): our own text, just enough of the third-party names for the reference's
// GroundSegmentation translation unit to compile unmodified and run (oracle/ref_build.py).  It is not the library it is named after,
// builds no other part of the reference and pins no third-party arithmetic (tools/pin/ does that).
// sensor_msgs/PointCloud2.h: the segmentation mentions no name of it; ros::NodeHandle and ROS_DEBUG_STREAM arrive through it.
#pragma once
#include <ros/ros.h>
