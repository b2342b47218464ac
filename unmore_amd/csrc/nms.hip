#pragma clang fp contract(off)
// Greedy non-maximum suppression of object discovery and object scoring (object_reasoning.py:661, object_scoring.py:238:
// torchvision.ops.nms(boxes, scores, iou_threshold)).  Rank r = position r of `order`, the caller's descending-score order.  Two
// launches on nms_bitmask.h, which states the specification: the upper triangle of the suppression matrix, no predicate, then one
// wave's greedy scan over all ranks with one word of removed set per lane (n <= 4096), no limit; keep[j] = order[rank of the j-th kept].
#include "umr_common.h"
#include "det_box.h"
#include "nms_bitmask.h"
#include <limits.h>

namespace {

constexpr int NMS_MAX_N = 4096;

__device__ __forceinline__ f32x4 nms_box(const float* __restrict__ boxes, const int64_t* __restrict__ order, int rank) {
    const float* b = boxes + order[rank] * 4;
    return f32x4{b[0], b[1], b[2], b[3]};
}

__global__ __launch_bounds__(64) void nms_tile_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ order, int n, float thresh,
                                                      unsigned long long* __restrict__ mat) {
    __shared__ f32x4 tile[64];
    const int rb = blockIdx.y, cbk = blockIdx.x, t = threadIdx.x, words = (n + 63) >> 6;
    if (cbk < rb) return;                                           // the upper triangle
    const int j0 = cbk * 64, nj = min(64, n - j0);
    if (t < nj) tile[t] = nms_box(boxes, order, j0 + t);
    __syncthreads();
    const int i = rb * 64 + t;
    if (i >= n) return;
    mat[(int64_t)i * words + cbk] = nms_tile_word(nms_box(boxes, order, i), i, tile, j0, nj, thresh, NmsAlways{});
}

__global__ __launch_bounds__(64) void nms_keep_kernel(const unsigned long long* __restrict__ mat, const int64_t* __restrict__ order, int n,
                                                      int64_t* __restrict__ keep, int32_t* __restrict__ n_keep) {
    __shared__ int kept_rank[NMS_MAX_N];
    const int lane = threadIdx.x, words = (n + 63) >> 6;
    const unsigned long long valid[1] = {nms_all_valid(lane, n)};
    const int kept = nms_greedy_scan<1>(mat, words, words, n, valid, INT_MAX, kept_rank);
    __syncthreads();
    for (int j = lane; j < kept; j += 64) keep[j] = order[kept_rank[j]];
    if (lane == 0) *n_keep = kept;
}

}  // namespace

extern "C" int64_t umr_nms_workspace(int n) { return n > 0 ? (int64_t)n * ((n + 63) / 64) * 8 : 0; }

extern "C" int umr_nms(const float* boxes, const int64_t* order, int n, float iou_threshold, void* workspace, int64_t workspace_bytes,
                       int64_t* keep, int32_t* n_keep, umr_stream_t stream) {
    UMR_CHECK_ARG(boxes && order && keep && n_keep && n > 0, "nms: bad arguments");
    if (n > NMS_MAX_N) return umr_set_error(UMR_ERR_UNSUPPORTED, "nms: at most 4096 boxes (one wave holds the removed set)");
    UMR_CHECK_ARG(workspace && workspace_bytes >= umr_nms_workspace(n) && ((uintptr_t)workspace & 7) == 0, "nms: workspace smaller than umr_nms_workspace(n) or misaligned");
    const int tiles = (n + 63) / 64;
    hipLaunchKernelGGL(nms_tile_kernel, dim3(tiles, tiles), dim3(64), 0, (hipStream_t)stream, boxes, order, n, iou_threshold,
                       (unsigned long long*)workspace);
    UMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(nms_keep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)workspace, order, n, keep, n_keep);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
