// Functional stand-in (TEST INFRASTRUCTURE): our own text, just enough of the third-party names for the reference's
// GroundSegmentation translation unit to compile unmodified and run (oracle/ref_build.py).  It is not the library it is named after,
// builds no other part of the reference and pins no third-party arithmetic (tools/pin/ does that).
// ros/ros.h: a NodeHandle that does nothing and ROS_DEBUG_STREAM as a no-op that still type-checks its argument.
#pragma once

#include <sstream>
#include <string>

namespace ros {
class NodeHandle {
public:
    NodeHandle() {}
    explicit NodeHandle(const std::string&) {}
};
struct Time {
    unsigned int sec = 0, nsec = 0;
};
} // namespace ros

#define ROS_DEBUG_STREAM(args)                \
    do {                                      \
        if (false) {                          \
            std::ostringstream gg_shim_ss_;   \
            gg_shim_ss_ << args;              \
        }                                     \
    } while (0)
