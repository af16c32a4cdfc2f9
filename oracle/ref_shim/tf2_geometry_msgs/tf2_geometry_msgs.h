// Functional stand-in (TEST INFRASTRUCTURE): our own text, just enough of the third-party names for the reference's
// GroundSegmentation translation unit to compile unmodified and run (oracle/ref_build.py).  It is not the library it is named after,
// builds no other part of the reference and pins no third-party arithmetic (tools/pin/ does that).
// tf2_geometry_msgs/tf2_geometry_msgs.h: tf2::doTransform(PointStamped).  The rotation matrix behind it is one of the unpinned
// conventions of tools/pin/README.md, written here from their description:
//   default                   KDL::Rotation::Quaternion (what tf2_geometry_msgs does in ROS Noetic): entries from the squares and
//                             doubled products of the quaternion's components; Frame * Vector = M * v + p, a row being
//                             (m0 * v0 + m1 * v1) + m2 * v2
//   -DGG_REF_SHIM_ROTATION_TF2  tf2::Matrix3x3::setRotation: s = 2 / |q|^2, entries from x * s, y * s, z * s; Transform * v = row . v + origin
#pragma once

#include <geometry_msgs/TransformStamped.h>

namespace tf2 {

inline void gg_shim_rotation(const geometry_msgs::Quaternion& q, double R[9])
{
    const double x = q.x, y = q.y, z = q.z, w = q.w;
#ifdef GG_REF_SHIM_ROTATION_TF2
    const double d = x * x + y * y + z * z + w * w;
    const double s = 2.0 / d;
    const double xs = x * s, ys = y * s, zs = z * s;
    const double wx = w * xs, wy = w * ys, wz = w * zs;
    const double xx = x * xs, xy = x * ys, xz = x * zs;
    const double yy = y * ys, yz = y * zs, zz = z * zs;
    R[0] = 1.0 - (yy + zz); R[1] = xy - wz;         R[2] = xz + wy;
    R[3] = xy + wz;         R[4] = 1.0 - (xx + zz); R[5] = yz - wx;
    R[6] = xz - wy;         R[7] = yz + wx;         R[8] = 1.0 - (xx + yy);
#else
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    R[0] = w2 + x2 - y2 - z2;     R[1] = 2 * x * y - 2 * w * z; R[2] = 2 * x * z + 2 * w * y;
    R[3] = 2 * x * y + 2 * w * z; R[4] = w2 - x2 + y2 - z2;     R[5] = 2 * y * z - 2 * w * x;
    R[6] = 2 * x * z - 2 * w * y; R[7] = 2 * y * z + 2 * w * x; R[8] = w2 - x2 - y2 + z2;
#endif
}

inline void doTransform(const geometry_msgs::PointStamped& t_in, geometry_msgs::PointStamped& t_out,
                        const geometry_msgs::TransformStamped& transform)
{
    double R[9];
    gg_shim_rotation(transform.transform.rotation, R);
    const double v[3] = {t_in.point.x, t_in.point.y, t_in.point.z};
    const double p[3] = {transform.transform.translation.x, transform.transform.translation.y, transform.transform.translation.z};
    double o[3];
    for (int r = 0; r < 3; ++r) o[r] = ((R[3 * r] * v[0] + R[3 * r + 1] * v[1]) + R[3 * r + 2] * v[2]) + p[r];
    t_out.point.x = o[0];
    t_out.point.y = o[1];
    t_out.point.z = o[2];
    t_out.header.stamp = transform.header.stamp;
    t_out.header.frame_id = transform.header.frame_id;
}

} // namespace tf2
