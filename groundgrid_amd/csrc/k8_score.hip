// K8 -- the evaluator's count (scripts/eval_groundpoint_classifier.py:95-132) on the device, behind the label loop.
//
// The reference's evaluation node receives the RETURNED cloud, in which `intensity` is 49 (predicted ground) / 99 (predicted non-ground)
// and `ring` carries the SemanticKITTI label (scripts/kitti_data_publisher.py:124-130), and counts per label id the points of either
// prediction; pc2.read_points(..., skip_nans=True) (:99) leaves out a point any of whose x, y, z is NaN.  Everything that needs is in
// HBM once k_label has run: the 2-bit label mask it wrote (gg_batch.d_label_masks, or the context's scratch when the caller passed none),
// `ring` in the input records, and the map-frame z -- a returned point is inside the map, so its x and y are finite, and z alone decides
// the NaN rule.  z is the record's own when the cloud came in the map frame, and rec's (K1's transformed height) when it did not.
//
// k_label decides 98 % of its labels from the cell and never re-reads the cloud, so this is a pass of its own and only launches that
// hold a scoring slot run it (gg_set_slot_scoring): same wave <-> chunk mapping as K1 / K5, four 64-point windows in flight, a
// histogram of at most 65 x 2 bins per work-group in LDS (one ds_add per RUN of equal bins in a window), then one 64-bit global atomic
// per non-zero bin and work-group.  Integer atomics: the result does not depend on arrival order.
//
// Algorithmic bytes per point: 16 (GG_POINT16; the sectors holding z and ring of a 32-byte point) + 0.25 (mask) read, + 8 (rec) for
// clouds that came with a transform.
#include "gg_device.h"

namespace gg {

template <int FMT>
__global__ __launch_bounds__(256) void k_score(const Arena a, const CloudParams *__restrict__ params, const BatchIO io, const ScoreArgs sc)
{
    const uint32_t item = xcd_contiguous_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int cloud = (int)(item / gridDim.x), bx = (int)(item % gridDim.x);
    const CloudParams cp = params[cloud];
    if (!sc.slot_on[cp.slot]) return; // (uniform over the work-group: a slot that does not score costs one byte)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunk = bx * 4 + wave;
    const int n = cp.n_points;

    __shared__ uint32_t hist[SCORE_BINS * 2]; // [bin][0 = predicted non-ground, 1 = predicted ground]; a chunk has fewer than 2^32 points
    for (int t = threadIdx.x; t < SCORE_BINS * 2; t += 256) hist[t] = 0u;
    __syncthreads();

    const int base = min(chunk * a.PW, n);
    const int end = min(base + a.PW, n);
    const char *pts = reinterpret_cast<const char *>(io.d_points) + (size_t)cp.io_index * io.cloud_stride * (FMT == GG_POINT16 ? 16 : 32);
    const uint2 *rec = a.rec + (size_t)cp.slot * a.point_stride;
    const uint8_t *masks = io.d_label_masks + (size_t)cp.io_index * ((io.cloud_stride + 3) / 4);
    const bool has_tf = cp.has_tf != 0;

    constexpr int ITEMS = 4;
    for (int p0 = base; p0 < end; p0 += 64 * ITEMS) {
        uint32_t zb[ITEMS], ring[ITEMS], mb[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) { // all windows' loads in flight together (unconditional, at clamped indices)
            const int p = min(p0 + j * 64 + lane, end - 1);
            if (FMT == GG_POINT16) {
                const uint2 v = *reinterpret_cast<const uint2 *>(pts + (size_t)p * 16 + 8); // z, ring | pad << 16
                zb[j] = v.x;
                ring[j] = v.y & 0xFFFFu;
            } else {
                zb[j] = *reinterpret_cast<const uint32_t *>(pts + (size_t)p * 32 + 8);
                ring[j] = *reinterpret_cast<const uint16_t *>(pts + (size_t)p * 32 + 20);
            }
            if (has_tf) zb[j] = rec[p].x; // the returned cloud is in the map frame
            mb[j] = masks[p >> 2];
        }
        uint32_t bin[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) bin[j] = sc.ring_bin[ring[j]];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int p = p0 + j * 64 + lane;
            const uint32_t code = (mb[j] >> (2 * (p & 3))) & 3u; // 0 dropped, 1 ground (49), 2 non-ground (99)
            const float z = __uint_as_float(zb[j]);
            const bool counts = p < end && code != 0u && !(z != z); // in the returned cloud, and read_points(skip_nans=True) keeps it
            const uint32_t id = counts ? bin[j] * 2u + (code == 1u ? 1u : 0u) : 0xFFFFu;
            const LaneRun run = lane_run(id, lane);
            if (run.head && counts) atomicAdd(&hist[id], (uint32_t)__popcll(run.mask));
        }
    }
    __syncthreads();
    unsigned long long *out = sc.scores + (size_t)cp.slot * SCORE_WORDS;
    for (int t = threadIdx.x; t < SCORE_BINS * 2; t += 256) {
        const uint32_t v = hist[t];
        if (v) atomicAdd(&out[1 + t], (unsigned long long)v);
    }
    if (bx == 0 && threadIdx.x == 0) atomicAdd(&out[0], 1ull); // gg_slot_scores::clouds
}

void launch_score(const Arena &a, const CloudParams *d_params, const BatchIO &io, const ScoreArgs &sc, int n_clouds, int max_n, hipStream_t s)
{
    if (n_clouds == 0) return;
    int nch = (max_n + a.PW - 1) / a.PW;
    if (nch == 0) nch = 1; // an empty cloud is still a cloud the evaluator received
    dim3 grid((nch + 3) / 4, n_clouds);
    if (io.point_format == GG_POINT16)
        hipLaunchKernelGGL((k_score<GG_POINT16>), grid, dim3(256), 0, s, a, d_params, io, sc);
    else
        hipLaunchKernelGGL((k_score<GG_POINT32>), grid, dim3(256), 0, s, a, d_params, io, sc);
}

} // namespace gg
