// arena_layout.h -- the one description of a context's device arena: which regions it holds, in which order, how large each is and which
// pointer and stride of Arena / ContextBuffers it defines.  Pure host arithmetic, no HIP runtime call: gg_create runs lay_out_arena twice,
// with a placer that only adds up the bytes (the size of the one hipMalloc) and with one that hands out base + offset, and
// tests/cpp/test_arena_layout.cpp runs it with a placer that records.  A placer is called as place(pointer, element_count): it owns
// the alignment (ARENA_ALIGN) and may leave the pointer alone.
#pragma once

#include <algorithm>

#include "gg_internal.h"

namespace gg {

#pragma GCC visibility push(hidden) // internal to the library: none of this joins its exported symbols

constexpr int PARAM_RING = 4;         // entries of a per-call parameter ring (gg_context.hip ParamRing)
constexpr size_t ARENA_ALIGN = 256;   // every region starts on a multiple of it

// what the layout depends on.  sweep_xchg_entries / sweep_pair_rec_floats are the results of the functions of those names (k4_sweep.hip,
// k4p_sweep_pair.hip), as plain values: this header links without the kernel files
struct ArenaShape {
    Geometry g;
    int n_slots;
    size_t max_points;
    int PW;            // points per wave chunk (Arena::PW, after GG_PW)
    int hist_pitch;    // words per chunk row of `hist` (Arena::hist_pitch)
    int gp_border_n;   // cells no sweep visits (ring >= c)
    bool k2_timing;    // GG_K2_DEBUG asks for k_reduce's phase counters: the k2_dbg region is K2_DBG_WGS * 32 words instead of 8
    bool sweep_timing; // GG_SWEEP_TIMING: ContextBuffers::d_sweep_dbg is set
    bool pair_timing;  // GG_PAIR_TIMING: Arena::pair_dbg is set
    size_t sweep_xchg_entries, sweep_pair_rec_floats;
};

// the context's own pointers into the arena (gg_context embeds it)
struct ContextBuffers {
    CloudParams *d_params = nullptr;  // [PARAM_RING][n_slots] the per-call parameter ring
    CloudParams *d_gparams = nullptr; // the one record a captured graph reads
    // staging of the host-buffer entry points
    gg_point16 *d_stage_pts = nullptr;
    uint8_t *d_stage_labels = nullptr;
    int32_t *d_stage_index = nullptr;
    int32_t *d_stage_counts = nullptr;
    uint8_t *d_stage_class = nullptr;
    int32_t *d_stage_cell = nullptr;
    // the async staging sets.  The results of one ticket are ONE block -- counts (64 B), then the index (4 n B), then the labels (n B) -- so
    // that they come back with a single copy; where the labels start inside it depends on the ticket's n
    struct AsyncSet {
        gg_point16 *d_pts = nullptr;
        uint8_t *d_results = nullptr;
        int32_t *d_counts = nullptr, *d_index = nullptr; // (= d_results, 64 bytes behind it)
    } async_set[GG_ASYNC_DEPTH];
    float *d_scroll_scratch = nullptr; // one layer in its device element order (map scroll) / two planes (images)
    float *d_image = nullptr;          // 3 * Cpad floats (wire-format images)
    float *d_bounds = nullptr;         // 2 floats
    unsigned long long *d_sweep_dbg = nullptr; // GG_SWEEP_TIMING=1: cycle counters of the sweep's wavefronts (cloud 0 of a batch)
    const ExportMap *d_slot_maps = nullptr;    // [n_slots]: entry s lists slot s alone -- the single-map getters' and setters' list of one map
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

template <class Placer> void lay_out_arena(Placer &place, const ArenaShape &in, Arena &a, ContextBuffers &b)
{
    const size_t A = ARENA_ALIGN, slots = (size_t)in.n_slots, N = in.max_points;
    const size_t C = (size_t)in.g.C, T = (size_t)in.g.T;
    const size_t Cpad = align_up(C * 4, A) / 4;
    // shared tables
    place(a.expected, C);
    place(a.patch_table, C);
    place(a.tile_rank, T);
    place(a.rank_tile, T);
    place(a.rank_cell0, T);
    // per slot
    a.slot_layer_stride = align_up(T * PERCALL_BLOCK * 4, A) / 4;
    place(a.layers, slots * a.slot_layer_stride);
    a.gpl = make_gp_layout(in.g.rows);
    // (a reserved region behind each slot's layer, gg_internal.h Arena::gp_bits: the slots keep the spacing they always had)
    a.gp_bits_off = (int)align_up((size_t)a.gpl.elems, 16);
    a.gp_bits_words = (a.gpl.elems / 64 + 2 + 1) & ~1; // (8-byte words, an even number)
    a.gp2_stride = align_up(((size_t)a.gp_bits_off + (size_t)a.gp_bits_words) * 8, A) / 8;
    a.gp_bits_stride = a.gp2_stride;
    place(a.gp2, slots * a.gp2_stride);
    if (a.gp2) a.gp_bits = reinterpret_cast<unsigned long long *>(a.gp2) + a.gp_bits_off;
    a.gp_fresh_cell = 1 + (a.gpl.VS - 1) * 64; // side 0, group 0, the last sheared position of ring 1: beyond the map's last column
    a.point_stride = align_up(N * 8, A) / 8;
    place(a.rec, slots * a.point_stride);
    place(a.sorted, slots * a.point_stride);
    a.zcell_stride = align_up((a.point_stride + 32 * T + 64) * 4, A) / 4;
    place(a.zcell, slots * a.zcell_stride);
    a.NCH = (int)((N + in.PW - 1) / in.PW);
    a.hist_stride = align_up((size_t)a.NCH * in.hist_pitch * 4, A) / 4;
    place(a.hist, slots * a.hist_stride);
    a.emit_stride = align_up((size_t)a.NCH * 4 * 4, A) / 4;
    place(a.chunk_emit, slots * a.emit_stride);
    place(a.totals, slots * 4);
    a.tile_start_stride = align_up((T + 1) * 4, A) / 4;
    place(a.tile_start, slots * a.tile_start_stride);
    a.tile_live_stride = align_up(T, A);
    place(a.tile_live, slots * a.tile_live_stride);
    a.tile_list_stride = align_up(T * 16, A) / 16;
    place(a.tile_list, slots * a.tile_list_stride);
    place(a.tile_list_cnt, slots * 2);
    // what the kernels synchronise through, each once more for the half of a batch that runs on the side stream
    place(a.front_sync, 2 * slots + 16);
    place(a.sweep_sync, 16);
    place(a.front_sync2, 2 * slots + 16);
    place(a.sweep_sync2, 16);
    place(a.scan_sync, slots * SCAN_SYNC_WORDS);
    place(a.scan_sync2, slots * SCAN_SYNC_WORDS);
    a.sweep_xchg_stride = align_up(std::max<size_t>(in.sweep_xchg_entries, 1) * 16, A) / 8;
    place(a.sweep_xchg, slots * a.sweep_xchg_stride);
    a.sweep_rec_stride = in.sweep_pair_rec_floats;
    a.sweep_rec_clouds = a.sweep_rec_stride ? std::min(in.n_slots, SWEEP_PAIR_MAX_CLOUDS) : 0;
    float *sweep_rec = nullptr;
    place(sweep_rec, std::max<size_t>((size_t)a.sweep_rec_clouds * a.sweep_rec_stride, 16));
    a.sweep_rec = a.sweep_rec_clouds ? sweep_rec : nullptr;
    // the context's parameter records and staging
    place(b.d_params, (size_t)PARAM_RING * slots);
    place(b.d_gparams, 1);
    place(b.d_stage_pts, N);
    place(b.d_stage_labels, N);
    place(b.d_stage_index, N);
    place(b.d_stage_counts, 16);
    place(b.d_stage_class, N);
    place(b.d_stage_cell, N);
    for (ContextBuffers::AsyncSet &as : b.async_set) {
        place(as.d_pts, N);
        place(as.d_results, 64 + N * 5 + 64);
        if (as.d_results) {
            as.d_counts = reinterpret_cast<int32_t *>(as.d_results);
            as.d_index = as.d_counts + 16;
        }
    }
    place(b.d_scroll_scratch, a.gp2_stride * 2);
    place(b.d_image, 3 * Cpad);
    place(b.d_bounds, 16);
    place(a.gp_valid, ((size_t)a.gpl.elems + 31) / 32);
    a.gp_border_n = in.gp_border_n;
    place(a.gp_border, std::max<size_t>((size_t)in.gp_border_n, 16));
    // the debug regions: carved either way, named only when their knob is set
    unsigned long long *sweep_dbg = nullptr, *pair_dbg = nullptr;
    place(sweep_dbg, 64);
    place(pair_dbg, 2048);
    b.d_sweep_dbg = in.sweep_timing ? sweep_dbg : nullptr;
    a.pair_dbg = in.pair_timing ? pair_dbg : nullptr;
    place(a.k2_dbg, in.k2_timing ? (size_t)K2_DBG_WGS * 32 : 8);
    place(b.d_slot_maps, slots);
}

// the two placers of gg_create: the byte count of the arena, and pointers into it
struct ArenaCounter {
    size_t bytes = 0;
    template <class T> void operator()(T *&, size_t count) { bytes = align_up(bytes + count * sizeof(T), ARENA_ALIGN); }
};
struct ArenaAssigner {
    char *base;
    size_t off = 0;
    template <class T> void operator()(T *&p, size_t count)
    {
        p = reinterpret_cast<T *>(base + off);
        off = align_up(off + count * sizeof(T), ARENA_ALIGN);
    }
};

#pragma GCC visibility pop

} // namespace gg
