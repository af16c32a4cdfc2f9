// ref_driver.cpp -- runs the reference's own GroundSegmentation translation unit on a scenario file (TEST INFRASTRUCTURE).
//
// What it is: our own text.  It includes the reference's src/GroundSegmentation.cpp BY PATH (GG_REFERENCE_SEGMENTATION_CPP, set by
// oracle/ref_build.py; the file is read where it lies, nothing of it is copied) so that the class and the detect_ground_patch<3> /
// <5> instantiations are compiled by a C++ compiler exactly as written, against the functional stand-ins of oracle/ref_shim/.
// What it is not: a build of the reference package, and no pin of the third-party arithmetic (tools/pin/ does that).
//
// One process per scenario: the reference binds function-local static references to the first map it sees (:76-78, :203-213,
// :317-321, :345-351, :447-452), so one process = one GridMap object = one geometry.
//
//   gg_ref_run <scenario> <results>
//
// Scenario (little-endian, fields in this order, see oracle/ref.py which writes it):
//   char[8] "GGREFSC1"; float length, resolution; double pos[2]; int32 point_count_cell_variance_threshold,
//   max_ring, thread_count; int32 n_steps; double cfg[11] (the double fields of GroundGridConfig in declaration order);
//   double quaternion[4] (x, y, z, w of the base transform); the layers the map starts with, in the order of kLayers below: a flag
//   byte per layer (11 bytes: 1 = the layer exists, all its rows * cols floats follow; 2 = it exists and is filled with the one float
//   that follows; 0 = it does not exist), each flag followed at once by its data; then n_steps steps: int32 op, int32 dump, arguments.
// The initial state of a map is DATA of the scenario: the driver knows no layer's initial value (oracle/ref.py sends what
// GroundGrid::initGroundGrid leaves, src/GroundGrid.cpp:55 and :71-75, or whatever a test supplies).
// Results: char[8] "GGREFRS1", int32 rows, cols, per step its outputs (below) and, if dump, a uint32 mask of the layers that exist and
// those layers; char[8] "GGREFEND" once every step ran.
#include GG_REFERENCE_SEGMENTATION_CPP

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

const char* const kLayers[11] = {"points", "ground", "groundpatch", "minGroundHeight", "maxGroundHeight", "groundCandidates",
                                 "planeDist", "m2", "meanVariance", "pointsRaw", "variance"};

enum Op { OP_FILTER = 1, OP_INSERT = 2, OP_DETECT_SECTION = 3, OP_SPIRAL = 4, OP_PATCH = 5, OP_INTERPOLATE = 6, OP_INIT = 7 };

typedef groundgrid::GroundSegmentation::PCLPoint PCLPoint;
static_assert(sizeof(PCLPoint) == 32 && alignof(PCLPoint) == 16, "PointXYZIR must be the 32-byte record");

// the protected table of init() (:40-46)
struct Segmentation : groundgrid::GroundSegmentation {
    const grid_map::Matrix& expected() const { return expectedPoints; }
};

FILE* g_in = nullptr;
FILE* g_out = nullptr;

void rd(void* p, size_t n)
{
    if (n && std::fread(p, 1, n, g_in) != n) {
        std::fprintf(stderr, "gg_ref_run: scenario ends early\n");
        std::exit(64);
    }
}
template <typename T> T rd()
{
    T v;
    rd(&v, sizeof(T));
    return v;
}
void wr(const void* p, size_t n)
{
    if (n && std::fwrite(p, 1, n, g_out) != n) {
        std::fprintf(stderr, "gg_ref_run: cannot write results\n");
        std::exit(65);
    }
}
template <typename T> void wr(const T& v) { wr(&v, sizeof(T)); }

void dump_layers(grid_map::GridMap& map)
{
    uint32_t mask = 0;
    for (int l = 0; l < 11; ++l)
        if (map.exists(kLayers[l])) mask |= 1u << l;
    wr(mask);
    for (int l = 0; l < 11; ++l)
        if (mask & (1u << l)) {
            const grid_map::Matrix& m = map[kLayers[l]];
            wr(m.data(), sizeof(float) * (size_t)m.size());
        }
}

pcl::PointCloud<PCLPoint>::Ptr read_cloud(uint64_t n)
{
    pcl::PointCloud<PCLPoint>::Ptr cloud(new pcl::PointCloud<PCLPoint>);
    cloud->points.resize(n);
    rd(cloud->points.data(), n * sizeof(PCLPoint));
    return cloud;
}

PCLPoint read_origin()
{
    PCLPoint o;
    std::memset(&o, 0, sizeof(o));
    float v[4];
    rd(v, sizeof(v));
    o.x = v[0];
    o.y = v[1];
    o.z = v[2];
    return o;
}

void write_pairs(const std::vector<std::pair<size_t, grid_map::Index>>& list)
{
    wr<uint64_t>(list.size());
    for (const auto& e : list) {
        wr<uint64_t>(e.first);
        wr<int32_t>(e.second(0));
        wr<int32_t>(e.second(1));
    }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <scenario> <results>\n", argv[0]);
        return 64;
    }
    g_in = std::fopen(argv[1], "rb");
    g_out = std::fopen(argv[2], "wb");
    if (!g_in || !g_out) {
        std::fprintf(stderr, "gg_ref_run: cannot open %s / %s\n", argv[1], argv[2]);
        return 66;
    }
    char magic[8];
    rd(magic, 8);
    if (std::memcmp(magic, "GGREFSC1", 8) != 0) {
        std::fprintf(stderr, "gg_ref_run: not a scenario file\n");
        return 64;
    }
    const float length = rd<float>(), resolution = rd<float>();
    double pos[2];
    rd(pos, sizeof(pos));
    groundgrid::GroundGridConfig cfg;
    cfg.point_count_cell_variance_threshold = rd<int32_t>();
    cfg.max_ring = rd<int32_t>();
    cfg.thread_count = rd<int32_t>();
    const int32_t n_steps = rd<int32_t>();
    double* const cfg_doubles[11] = {&cfg.groundpatch_detection_minimum_threshold, &cfg.distance_factor, &cfg.minimum_distance_factor,
                                     &cfg.miminum_point_height_threshold, &cfg.minimum_point_height_obstacle_threshold,
                                     &cfg.outlier_tolerance, &cfg.ground_patch_detection_minimum_point_count_threshold,
                                     &cfg.patch_size_change_distance, &cfg.occupied_cells_decrease_factor,
                                     &cfg.occupied_cells_point_count_factor, &cfg.min_outlier_detection_ground_confidence};
    for (double* d : cfg_doubles) *d = rd<double>();
    double quat[4];
    rd(quat, sizeof(quat));

    // geometry first (float members handed to double parameters, as at src/GroundGrid.cpp:58), then the scenario's layers
    grid_map::GridMap map;
    const grid_map::Length side(length, length);
    const grid_map::Position centre(pos[0], pos[1]);
    map.setGeometry(side, static_cast<double>(resolution), centre);
    const int rows = map.getSize()(0), cols = map.getSize()(1);
    for (int l = 0; l < 11; ++l) {
        const uint8_t flag = rd<uint8_t>();
        if (flag == 0) continue;
        grid_map::Matrix m(rows, cols);
        if (flag == 2)
            m.setConstant(rd<float>());
        else
            rd(m.data(), sizeof(float) * (size_t)m.size());
        map.add(kLayers[l], m);
    }

    Segmentation seg;
    ros::NodeHandle nh;
    seg.setConfig(cfg);
    seg.init(nh, length, resolution); // src/GroundGridNodelet.cpp:95: the float dimension goes into a size_t parameter

    wr("GGREFRS1", 8);
    wr<int32_t>(rows);
    wr<int32_t>(cols);

    for (int32_t s = 0; s < n_steps; ++s) {
        const int32_t op = rd<int32_t>(), dump = rd<int32_t>();
        switch (op) {
        case OP_FILTER: { // -> uint64 n_out, the returned cloud
            const uint64_t n = rd<uint64_t>();
            const PCLPoint origin = read_origin();
            geometry_msgs::TransformStamped to_base;
            to_base.header.frame_id = "base_link";
            to_base.transform.translation.z = rd<double>();
            to_base.transform.rotation.x = quat[0];
            to_base.transform.rotation.y = quat[1];
            to_base.transform.rotation.z = quat[2];
            to_base.transform.rotation.w = quat[3];
            const pcl::PointCloud<PCLPoint>::Ptr cloud = read_cloud(n);
            const pcl::PointCloud<PCLPoint>::Ptr out = seg.filter_cloud(cloud, origin, to_base, map);
            wr<uint64_t>(out->points.size());
            wr(out->points.data(), out->points.size() * sizeof(PCLPoint));
            break;
        }
        case OP_INSERT: { // -> the three lists insert_cloud appends: (point, row, col) kept, (point, row, col) ignored, outliers
            const uint64_t n = rd<uint64_t>(), start = rd<uint64_t>(), end = rd<uint64_t>();
            const PCLPoint origin = read_origin();
            const pcl::PointCloud<PCLPoint>::Ptr cloud = read_cloud(n);
            std::vector<std::pair<size_t, grid_map::Index>> kept_list, ignored_list;
            std::vector<size_t> outlier_list;
            seg.insert_cloud(cloud, start, end, origin, kept_list, ignored_list, outlier_list, map);
            write_pairs(kept_list);
            write_pairs(ignored_list);
            wr<uint64_t>(outlier_list.size());
            for (size_t i : outlier_list) wr<uint64_t>(i);
            break;
        }
        case OP_DETECT_SECTION:
            seg.detect_ground_patches(map, (unsigned short)rd<int32_t>());
            break;
        case OP_SPIRAL: {
            geometry_msgs::TransformStamped to_base;
            to_base.transform.translation.z = rd<double>();
            to_base.transform.rotation.x = quat[0];
            to_base.transform.rotation.y = quat[1];
            to_base.transform.rotation.z = quat[2];
            to_base.transform.rotation.w = quat[3];
            seg.spiral_ground_interpolation(map, to_base);
            break;
        }
        case OP_PATCH: {
            const int32_t S = rd<int32_t>();
            const uint64_t i = rd<uint64_t>(), j = rd<uint64_t>();
            if (S == 3)
                seg.detect_ground_patch<3>(map, i, j);
            else
                seg.detect_ground_patch<5>(map, i, j);
            break;
        }
        case OP_INTERPOLATE: {
            const uint64_t x = rd<uint64_t>(), y = rd<uint64_t>();
            seg.interpolate_cell(map, x, y);
            break;
        }
        case OP_INIT: // -> expectedPoints
            wr(seg.expected().data(), sizeof(float) * (size_t)seg.expected().size());
            break;
        default:
            std::fprintf(stderr, "gg_ref_run: unknown step %d\n", op);
            return 64;
        }
        if (dump) dump_layers(map);
        std::fflush(g_out);
    }
    wr("GGREFEND", 8);
    std::fclose(g_out);
    return 0;
}
