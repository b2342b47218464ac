// One axis of torchvision's roi_align(aligned=True) as mask_loss.hip and roi_pool.hip walk it: the sample coordinate, the run of a bin's
// samples that fall inside [-1, size], and a sample's taps.  float32, no contraction: include only after `#pragma clang fp contract(off)`.
#pragma once
#include "umr_common.h"

// coordinate(p, i) = (start + (p * bin)) + (((i + .5f) * bin) / grid), the division correctly rounded
__device__ __forceinline__ float roi_axis_coord(float start, float bin, int grid, int p, int i) {
    return start + (float)p * bin + __fdiv_rn(((float)i + .5f) * bin, (float)grid);
}

// the first i in [0, grid] with coordinate(p, i) >= bound (strict: > bound); the coordinate does not decrease with i
__device__ __forceinline__ int roi_axis_first(float start, float bin, int grid, int p, float bound, bool strict) {
    int lo = 0, hi = grid;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const float c = roi_axis_coord(start, bin, grid, p, mid);
        if (strict ? c > bound : c >= bound) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// (low tap, bits of the fraction), low = -1 for a sample outside [-1, size]; 0 <= low <= size - 1 otherwise
__device__ __forceinline__ int2 roi_axis_entry(float c, int size) {
    if (!(c >= -1.f && c <= (float)size)) return make_int2(-1, 0);
    if (c <= 0.f) c = 0.f;
    int low = (int)c;
    if (low >= size - 1) { low = size - 1; c = (float)low; }
    return make_int2(low, __float_as_int(c - (float)low));
}
