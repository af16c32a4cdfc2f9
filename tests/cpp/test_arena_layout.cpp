// Host-side check of the device arena's layout (groundgrid_amd/csrc/arena_layout.h): lay_out_arena is run with a placer that records every
// region, for three geometries x three context sizes x both wave-chunk sizes x the debug knobs off and on.  Every region is 256-byte
// aligned, the regions are disjoint and in order, the counted total ends the last one, every region holds what its consumers address, and
// the counting and the assigning placer of gg_create agree with the record.  Compiled host-only by tests/test_arena_layout_cpu.py and linked with the built library.
//   test_arena_layout          prints "ok" or the first violation
//   test_arena_layout --json   prints the (region, offset, bytes) table of every configuration (profiles/context_lifetime/arena_offsets.json)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "arena_layout.h"
#include "scroll_core.h"
#include "sweep_core.h"

using namespace gg;

// the regions in the order lay_out_arena places them (the placer is told no names: the record numbers its calls); the two async_* repeat
// GG_ASYNC_DEPTH times
static const char *const HEAD[] = {"expected", "patch_table", "tile_rank", "rank_tile", "rank_cell0", "layers", "gp2", "rec", "sorted", "zcell", "hist",
                                   "chunk_emit", "totals", "tile_start", "tile_live", "tile_list", "tile_list_cnt", "front_sync", "sweep_sync", "front_sync2",
                                   "sweep_sync2", "scan_sync", "scan_sync2", "sweep_xchg", "sweep_rec", "d_params", "d_gparams", "d_stage_pts", "d_stage_labels",
                                   "d_stage_index", "d_stage_counts", "d_stage_class", "d_stage_cell"};
static const char *const ASYNC[] = {"async_pts", "async_results"};
static const char *const TAIL[] = {"d_scroll_scratch", "d_image", "d_bounds", "gp_valid", "gp_border", "sweep_dbg", "pair_dbg", "k2_dbg", "d_slot_maps"};
static std::vector<std::string> region_names()
{
    std::vector<std::string> v(HEAD, HEAD + sizeof HEAD / sizeof *HEAD);
    for (int k = 0; k < GG_ASYNC_DEPTH; ++k) v.insert(v.end(), ASYNC, ASYNC + 2);
    v.insert(v.end(), TAIL, TAIL + sizeof TAIL / sizeof *TAIL);
    return v;
}

struct Region {
    std::string name;
    size_t offset, bytes;
    const void *ptr;
};
struct Recorder {
    char *base;
    size_t off = 0;
    std::vector<Region> regions;
    template <class T> void operator()(T *&p, size_t count)
    {
        p = reinterpret_cast<T *>(base + off);
        regions.push_back({"", off, count * sizeof(T), p});
        off = align_up(off + count * sizeof(T), ARENA_ALIGN);
    }
};

static ArenaShape make_shape(float length, float resolution, int n_slots, size_t max_points, int PW, bool knobs)
{
    const int n = (int)round((double)length / (double)resolution); // (gg_create)
    ArenaShape s{};
    s.g.rows = s.g.cols = n;
    s.g.C = n * n;
    s.g.tiles_r = s.g.tiles_c = (n + TILE - 1) / TILE;
    s.g.T = s.g.tiles_r * s.g.tiles_c;
    s.n_slots = n_slots;
    s.max_points = max_points;
    s.PW = PW;
    s.hist_pitch = (s.g.T + 3) & ~3;
    const GpLayout L = make_gp_layout(n);
    for (int col = 0; col < n; ++col)
        for (int row = 0; row < n; ++row)
            if (std::max(std::abs(row - L.c), std::abs(col - L.c)) >= L.c) ++s.gp_border_n;
    s.k2_timing = s.sweep_timing = s.pair_timing = knobs;
    // the sweep's two sizes, from the library's own functions as gg_create calls them (the program links the built library: host code only)
    gg_geometry geom;
    gg_default_geometry(&geom);
    gg_config cfg;
    gg_default_config(&cfg);
    const sweep::Params sp = sweep::make_params(n, (double)resolution, geom.min_dist_squared, cfg.occupied_cells_decrease_factor);
    s.sweep_xchg_entries = sweep_xchg_entries(sp);
    s.sweep_pair_rec_floats = sweep_pair_rec_floats(sp);
    return s;
}

// what the consumers of each region address, in bytes
static std::map<std::string, size_t> needs(const ArenaShape &s, const Arena &a)
{
    const size_t S = (size_t)s.n_slots, N = s.max_points, C = (size_t)s.g.C, T = (size_t)s.g.T, Cpad = (C * 4 + 255) / 256 * 64;
    std::map<std::string, size_t> m;
    m["expected"] = C * 4;
    m["patch_table"] = C * 16;
    m["tile_rank"] = m["rank_tile"] = T * 2;
    m["rank_cell0"] = T * 4;
    m["layers"] = S * a.slot_layer_stride * 4;
    m["gp2"] = S * a.gp2_stride * 8;
    m["rec"] = m["sorted"] = S * a.point_stride * 8;
    m["zcell"] = S * a.zcell_stride * 4;
    m["hist"] = S * a.hist_stride * 4;
    m["chunk_emit"] = S * a.emit_stride * 4;
    m["totals"] = S * 4 * 4;
    m["tile_start"] = S * a.tile_start_stride * 4;
    m["tile_live"] = S * a.tile_live_stride * 4;
    m["tile_list"] = S * a.tile_list_stride * 16;
    m["tile_list_cnt"] = S * 2 * 4;
    m["front_sync"] = m["front_sync2"] = (2 * S + 16) * 4;
    m["sweep_sync"] = m["sweep_sync2"] = 4 * 4;
    m["scan_sync"] = m["scan_sync2"] = S * SCAN_SYNC_WORDS * 8;
    m["sweep_xchg"] = S * a.sweep_xchg_stride * 8;
    m["sweep_rec"] = (size_t)a.sweep_rec_clouds * a.sweep_rec_stride * 4;
    m["d_params"] = (size_t)PARAM_RING * S * sizeof(CloudParams);
    m["d_gparams"] = sizeof(CloudParams);
    m["d_stage_pts"] = m["async_pts"] = N * sizeof(gg_point16);
    m["d_stage_labels"] = m["d_stage_class"] = N;
    m["d_stage_index"] = m["d_stage_cell"] = N * 4;
    m["d_stage_counts"] = 16;
    m["async_results"] = 64 + N * 4 + N; // counts, index, labels
    m["d_scroll_scratch"] = std::max((size_t)a.gpl.elems * 8, 2 * C * 4); // one layer in element order / two planes
    m["d_image"] = 3 * Cpad * 4;
    m["d_bounds"] = 2 * 4;
    m["gp_valid"] = ((size_t)a.gpl.elems + 31) / 32 * 4;
    m["gp_border"] = (size_t)s.gp_border_n * 4;
    m["sweep_dbg"] = 64 * 8;
    m["pair_dbg"] = 2048 * 8;
    m["k2_dbg"] = s.k2_timing ? (size_t)K2_DBG_WGS * 32 * 8 : 8;
    m["d_slot_maps"] = S * sizeof(ExportMap);
    return m;
}

int main(int argc, char **argv)
{
    const bool json = argc > 1 && !strcmp(argv[1], "--json");
    const float geoms[3][2] = {{120.f, .33f}, {20.f, .33f}, {61.f, .25f}};
    const size_t sizes[3][2] = {{1, 64}, {3, 5000}, {1024, 131072}};
    char *const base = reinterpret_cast<char *>((uintptr_t)1 << 40); // never dereferenced
    if (json) printf("[");
    bool first = true;
    for (const auto &gm : geoms)
        for (const auto &sz : sizes)
            for (const int PW : {1024, 2048})
                for (const bool knobs : {false, true}) {
                    const ArenaShape s = make_shape(gm[0], gm[1], (int)sz[0], sz[1], PW, knobs);
                    char cfg[160];
                    snprintf(cfg, sizeof cfg, "length %g resolution %g n_slots %zu max_points %zu PW %d knobs %d", gm[0], gm[1], sz[0], sz[1], PW, (int)knobs);
                    Arena a{}, a0{}, a2{};
                    ContextBuffers b, b0, b2;
                    Recorder rec{base};
                    lay_out_arena(rec, s, a, b);
                    const std::vector<std::string> names = region_names();
                    if (names.size() != rec.regions.size()) return printf("%s: %zu regions placed, the test names %zu\n", cfg, rec.regions.size(), names.size()), 1;
                    for (size_t k = 0; k < names.size(); ++k) rec.regions[k].name = names[k];
                    ArenaCounter count;
                    lay_out_arena(count, s, a0, b0);
                    ArenaAssigner assign{base};
                    lay_out_arena(assign, s, a2, b2);
                    if (json) {
                        if (knobs) continue; // (the knobs change no offset but k2_dbg's size: checked below, not tabulated)
                        printf("%s\n{\"length\": %g, \"resolution\": %g, \"n_slots\": %zu, \"max_points\": %zu, \"PW\": %d, \"arena_bytes\": %zu, \"regions\": [", first ? "" : ",", gm[0],
                               gm[1], sz[0], sz[1], PW, count.bytes);
                        for (size_t k = 0; k < rec.regions.size(); ++k)
                            printf("%s[\"%s\", %zu, %zu]", k ? ", " : "", rec.regions[k].name.c_str(), rec.regions[k].offset, rec.regions[k].bytes);
                        printf("]}");
                        first = false;
                        continue;
                    }
                    const std::map<std::string, size_t> need = needs(s, a);
                    // a slot's share of every strided region holds what the kernels keep there per slot
                    const size_t T = (size_t)s.g.T, N = s.max_points;
                    if (a.slot_layer_stride < T * PERCALL_BLOCK || a.gp2_stride < (size_t)a.gp_bits_off + (size_t)a.gp_bits_words || a.point_stride < N ||
                        a.zcell_stride < N + 32 * T + 64 || (size_t)a.NCH * PW < N || a.hist_stride < (size_t)a.NCH * s.hist_pitch || (size_t)s.hist_pitch < T ||
                        a.emit_stride < (size_t)a.NCH * 4 || a.tile_start_stride < T + 1 || a.tile_live_stride < T || a.tile_list_stride < T ||
                        a.sweep_xchg_stride * 8 < s.sweep_xchg_entries * 16)
                        return printf("%s: a per-slot stride is smaller than what a slot holds\n", cfg), 1;
                    size_t end = 0;
                    std::map<std::string, int> seen;
                    for (const Region &r : rec.regions) {
                        if (r.offset % 256) return printf("%s: %s is not 256-byte aligned\n", cfg, r.name.c_str()), 1;
                        if (r.offset < end) return printf("%s: %s overlaps the region in front of it\n", cfg, r.name.c_str()), 1; // (in order: pairwise disjoint)
                        end = r.offset + r.bytes;
                        if (end > count.bytes) return printf("%s: %s ends behind the counted total\n", cfg, r.name.c_str()), 1;
                        const auto it = need.find(r.name);
                        if (it == need.end()) return printf("%s: %s has no consumer size in this test\n", cfg, r.name.c_str()), 1;
                        if (r.bytes < it->second) return printf("%s: %s holds %zu bytes, its consumers address %zu\n", cfg, r.name.c_str(), r.bytes, it->second), 1;
                        ++seen[r.name];
                    }
                    for (const auto &kv : need)
                        if (seen[kv.first] != (kv.first.rfind("async_", 0) == 0 ? GG_ASYNC_DEPTH : 1)) return printf("%s: %s placed %d times\n", cfg, kv.first.c_str(), seen[kv.first]), 1;
                    if (align_up(end, 256) != count.bytes || rec.off != count.bytes || assign.off != count.bytes)
                        return printf("%s: counted %zu, recorded %zu, assigned %zu, last region ends at %zu\n", cfg, count.bytes, rec.off, assign.off, end), 1;
                    // the counting pass defines the same strides and touches no pointer; the assigning pass gives the recorded pointers
                    if (a0.gp2 || a0.gp_bits || a0.sweep_rec || a0.k2_dbg || b0.d_params || b0.async_set[0].d_index || b0.d_slot_maps)
                        return printf("%s: the counting pass set a pointer\n", cfg), 1;
                    if (a0.gp2_stride != a.gp2_stride || a0.zcell_stride != a.zcell_stride || a0.hist_stride != a.hist_stride || a0.NCH != a.NCH ||
                        a0.sweep_xchg_stride != a.sweep_xchg_stride || a0.tile_list_stride != a.tile_list_stride || a0.slot_layer_stride != a.slot_layer_stride)
                        return printf("%s: the two passes disagree about a stride\n", cfg), 1;
                    const std::pair<const char *, const void *> assigned[] = {{"expected", a2.expected}, {"patch_table", a2.patch_table}, {"tile_rank", a2.tile_rank},
                        {"rank_tile", a2.rank_tile}, {"rank_cell0", a2.rank_cell0}, {"layers", a2.layers}, {"gp2", a2.gp2}, {"rec", a2.rec}, {"sorted", a2.sorted},
                        {"zcell", a2.zcell}, {"hist", a2.hist}, {"chunk_emit", a2.chunk_emit}, {"totals", a2.totals}, {"tile_start", a2.tile_start},
                        {"tile_live", a2.tile_live}, {"tile_list", a2.tile_list}, {"tile_list_cnt", a2.tile_list_cnt}, {"front_sync", a2.front_sync},
                        {"sweep_sync", a2.sweep_sync}, {"front_sync2", a2.front_sync2}, {"sweep_sync2", a2.sweep_sync2}, {"scan_sync", a2.scan_sync},
                        {"scan_sync2", a2.scan_sync2}, {"sweep_xchg", a2.sweep_xchg}, {"d_params", b2.d_params}, {"d_gparams", b2.d_gparams},
                        {"d_stage_pts", b2.d_stage_pts}, {"d_stage_labels", b2.d_stage_labels}, {"d_stage_index", b2.d_stage_index},
                        {"d_stage_counts", b2.d_stage_counts}, {"d_stage_class", b2.d_stage_class}, {"d_stage_cell", b2.d_stage_cell},
                        {"async_pts", b2.async_set[0].d_pts}, {"async_results", b2.async_set[0].d_counts}, {"d_scroll_scratch", b2.d_scroll_scratch},
                        {"d_image", b2.d_image}, {"d_bounds", b2.d_bounds}, {"gp_valid", a2.gp_valid}, {"gp_border", a2.gp_border}, {"k2_dbg", a2.k2_dbg},
                        {"d_slot_maps", b2.d_slot_maps}};
                    for (const auto &p : assigned)
                        for (const Region &r : rec.regions)
                            if (r.name == p.first) {
                                if (r.ptr != p.second) return printf("%s: the assigning pass put %s elsewhere\n", cfg, p.first), 1;
                                break; // (the first of the async sets)
                            }
                    // derived and conditional pointers
                    const size_t bits_end = ((size_t)a2.gp_bits_off + (size_t)a2.gp_bits_words) * 8;
                    if ((const char *)a2.gp_bits != (const char *)a2.gp2 + (size_t)a2.gp_bits_off * 8 || (size_t)a2.gp_bits_off < (size_t)a2.gpl.elems || bits_end > a2.gp2_stride * 8 ||
                        (size_t)a2.gp_bits_words * 64 < (size_t)a2.gpl.elems)
                        return printf("%s: gp_bits does not sit inside the slot's gp2 region behind its elements\n", cfg), 1;
                    for (const ContextBuffers::AsyncSet &as : b2.async_set)
                        if ((const void *)as.d_counts != as.d_results || as.d_index != as.d_counts + 16) return printf("%s: an async set's index is not 64 bytes behind its counts\n", cfg), 1;
                    if ((a2.sweep_rec != nullptr) != (a2.sweep_rec_clouds > 0) || (a2.pair_dbg != nullptr) != knobs || (b2.d_sweep_dbg != nullptr) != knobs)
                        return printf("%s: a conditional pointer does not follow its condition\n", cfg), 1;
                }
    printf(json ? "\n]\n" : "ok\n");
    return 0;
}
