// The k largest keys of a sequence, equal keys in sequence order, handed out in sequence order: a four-pass radix select over 8-bit
// digits, templated on where the keys come from and on what is done with a selected entry.  Used by rpn.hip (per-level top-k of the
// scores), rpn_loss.hip (the anchor batch) and roi_sample.hip (the proposal batch).
//
// Src gives `unsigned key(Index i) const`, Index the integer type of the length n (int or int64_t): the loops count in it.  A key of
// 0 marks an entry that takes no part: it is never counted and never handed out, so a caller selects among a subset of the sequence
// by giving the others 0 and its own entries keys >= 1.  k >= 1; when fewer than k entries have a non-zero key, all of them are
// selected.
#pragma once
#include "umr_common.h"

// Every thread of the workgroup calls it (blockDim.x a multiple of 64, at most 1024); hist: 256 ints, wtot: 2 * 16 ints of LDS.
// emit(j, i, key) is called once, by the thread that holds it, for the j-th selected entry in ascending sequence index i, j < the
// returned count (min(k, entries with a non-zero key), the same in every thread).  What emit stores, in LDS or memory, is complete
// after the call's final barrier.
template <typename Src, typename Index, typename Emit>
__device__ int select_in_order(const Src& src, Index n, int k, int* hist, int* wtot, Emit emit) {
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = T >> 6;
    unsigned prefix = 0u, mask = 0u;
    int remaining = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();
        for (int b = tid; b < 256; b += T) hist[b] = 0;
        __syncthreads();
        for (Index i = tid; i < n; i += T) {
            const unsigned key = src.key(i);
            if (key && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        int cum = 0, digit = -1;
        for (int b = 255; b >= 0; --b) {                            // every thread walks the same histogram
            const int h = hist[b];
            if (cum + h >= remaining) { digit = b; break; }
            cum += h;
        }
        if (digit < 0) {                                            // (first pass only) fewer than k entries take part: all of them
            prefix = 0u;
            remaining = 0;
            break;
        }
        remaining -= cum;
        prefix |= (unsigned)digit << shift;
        mask |= 255u << shift;
    }
    // prefix: the k-th largest key; `remaining` >= 1 of the keys equal to it are taken, the first ones (or prefix 0 and none: all)
    int n_gt = 0, n_eq = 0, par = 0;
    for (Index base = 0; base < n; base += T) {
        const Index i = base + tid;
        unsigned key = 0u;
        bool gt = false, eq = false;
        if (i < n) {
            key = src.key(i);
            gt = key > prefix;
            eq = key == prefix && key != 0u;
        }
        const unsigned long long vg = __ballot(gt), ve = __ballot(eq);
        if (lane == 0) wtot[par * 16 + wv] = __popcll(vg) | (__popcll(ve) << 8);
        __syncthreads();
        const unsigned long long below = (1ull << lane) - 1ull;
        int g = n_gt + __popcll(vg & below), e = n_eq + __popcll(ve & below), tg = 0, te = 0;
        for (int w = 0; w < nw; ++w) {
            const int v = wtot[par * 16 + w];
            if (w < wv) { g += v & 255; e += v >> 8; }
            tg += v & 255;
            te += v >> 8;
        }
        if (gt || (eq && e < remaining)) {
            const int at = g + min(e, remaining);
            if (at >= 0 && at < k) emit(at, i, key);                // always
        }
        n_gt += tg;
        n_eq += te;
        par ^= 1;
    }
    __syncthreads();
    return n_gt + min(n_eq, remaining);
}

// the emit that keeps the sequence index alone: out[j] = i
struct SelectStoreIndex {
    int32_t* out;
    __device__ __forceinline__ void operator()(int j, int64_t i, unsigned) const { out[j] = (int32_t)i; }
};
