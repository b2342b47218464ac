// The finishing sum of a backward kernel that leaves one float32 record of partial sums per workgroup: out[e] = sum over the records
// i < n of partials[i * stride + e], for the elements e < total, in an order that is a function of n alone.  Used by mask_head.hip
// (records [C + 1]: dwp | dbp) and rpn_head.hip (records [16][C + 1], of which the first 5A rows count: dwo | dbo | dwd | dbd).
//
// A workgroup of 1024 threads takes the elements 64 * blockIdx.x .. + 63, lane l of every wave element 64 * blockIdx.x + l, so a wave
// reads 256 consecutive bytes of a record.  Wave w of 16 adds the records w, w + 16, ... in index order into one float; the 16 waves'
// sums meet in LDS and wave 0 adds them in wave order, red[l] + red[64 + l] + ... + red[15 * 64 + l] left to right.  No float
// atomics: the same records give the same bytes on every run.  n == 0 stores zeros.
//
// Store: `void operator()(int e, float v) const`, called once per element by the lane that holds its sum: where element e goes.
// Launch: <<<(total + 63) / 64, FINISH_THREADS, 0, stream>>>.
#pragma once
#include "umr_common.h"

constexpr int FINISH_THREADS = 1024;

template <typename Store>
__global__ __launch_bounds__(FINISH_THREADS) void finish_partials_kernel(const float* __restrict__ partials, int64_t n, int64_t stride,
                                                                         int total, Store store) {
    __shared__ float red[FINISH_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int e = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (e < total)
        for (int64_t i = wv; i < n; i += FINISH_THREADS / 64) s += partials[i * stride + e];
    red[tid] = s;
    __syncthreads();
    if (wv == 0 && e < total) {
        float t = red[lane];
        for (int k = 1; k < FINISH_THREADS / 64; ++k) t += red[k * 64 + lane];
        store(e, t);
    }
}
