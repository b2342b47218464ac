// The back end of the COCO run-length encoders (rle.hip, poly_rle.hip): an ordered stream of positions with a 0/1 value each ->
// the run boundaries -> the deltas -> the 5-bit groups of pycocotools' string format, as a measure pass (sizes) or a packed write pass.
// A producer P gives value(p) in {0,1}, before() (the pixel preceding position 0 of its stream) and gpos(p), the position in the
// mask's column-major order (increasing in p).  One workgroup of RLE_THREADS threads per mask; rle.hip's header describes the chunking.
#pragma once
#include "umr_common.h"

namespace {

constexpr int RLE_THREADS = 256, RLE_E = 8, RLE_WAVE_SPAN = 64 * RLE_E, RLE_CHUNK = RLE_THREADS * RLE_E;

struct RleShared {
    uint32_t lst[RLE_CHUNK + 3];      // [0..2] = the three boundaries before this chunk's, then this chunk's in stream order
    uint32_t wtot[2][4];              // flags per wave, double-buffered by chunk parity (a chunk without flags has one barrier only)
    uint32_t stot[4];                 // character-scan wave totals
};
struct RleState {                     // the same in every thread of the workgroup
    uint32_t nb = 1;                  // boundaries so far (b[0] = 0 is the start of run 0) == runs opened
    uint32_t b1 = 0, b2 = 0, b3 = 0;  // b[nb-1], b[nb-2], b[nb-3]
    int64_t nchars = 0;
    int par = 0;
};

__device__ __forceinline__ int rle_nchars(int32_t x) {
    int n = 0;
    bool more;
    do {
        const int c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        ++n;
    } while (more);
    return n;
}
__device__ __forceinline__ void rle_emit(int32_t x, uint8_t* __restrict__ out, int64_t off, int64_t end) {
    bool more;
    do {
        int c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        if (off < end) out[off] = (uint8_t)(c + 48);      // `end`: the caller's capacity -- wrong offsets cannot write past the buffer
        ++off;
    } while (more);
}
// the value run i is written as, from its closing boundary b and the three before it
__device__ __forceinline__ int32_t rle_delta(uint32_t i, uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3) {
    const int32_t cnt = (int32_t)(b - p1);
    return i > 2 ? cnt - (int32_t)(p2 - p3) : cnt;
}

// Streams n_local positions of producer P through the back end.  P: value(p) in {0,1}; before(): the pixel preceding position 0 of
// this stream; gpos(p): the position in the mask's column-major order (increasing in p).  Called by every thread of the workgroup.
template <bool WRITE, typename P>
__device__ __forceinline__ void rle_stream(const P& prod, uint32_t n_local, RleShared& sh, RleState& st, uint8_t* __restrict__ out, int64_t out_base,
                                           int64_t out_end) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t cb = 0; cb < n_local; cb += RLE_CHUNK) {
        const uint32_t wb0 = cb + (uint32_t)w * RLE_WAVE_SPAN;
        int carry = 0;
        if (lane == 0 && wb0 < n_local) carry = wb0 == 0 ? prod.before() : prod.value(wb0 - 1);
        unsigned fm = 0;
        uint32_t wcount = 0;
#pragma unroll
        for (int e = 0; e < RLE_E; ++e) {
            const uint32_t p = wb0 + (uint32_t)e * 64 + lane;
            const bool valid = p < n_local;
            const int v = valid ? prod.value(p) : 0;
            const int up = __shfl_up(v, 1, 64);
            const int prev = lane == 0 ? carry : up;
            carry = __shfl(v, 63, 64);
            const bool flag = valid && v != prev;
            fm |= (flag ? 1u : 0u) << e;
            wcount += (uint32_t)__popcll(__ballot(flag));
        }
        if (lane == 0) sh.wtot[st.par][w] = wcount;
        __syncthreads();
        const uint32_t t0 = sh.wtot[st.par][0], t1 = sh.wtot[st.par][1], t2 = sh.wtot[st.par][2], t3 = sh.wtot[st.par][3];
        st.par ^= 1;
        const uint32_t T = t0 + t1 + t2 + t3;
        if (T == 0) continue;                                   // workgroup-uniform
        uint32_t rank = (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
        if (tid < 3) sh.lst[tid] = tid == 0 ? st.b3 : tid == 1 ? st.b2 : st.b1;
#pragma unroll
        for (int e = 0; e < RLE_E; ++e) {
            const bool flag = (fm >> e) & 1u;
            const unsigned long long ball = __ballot(flag);
            if (flag) sh.lst[3 + rank + (uint32_t)__popcll(ball & lt)] = prod.gpos(wb0 + (uint32_t)e * 64 + lane);
            rank += (uint32_t)__popcll(ball);
        }
        __syncthreads();
        for (uint32_t base = 0; base < T; base += RLE_THREADS) {
            const uint32_t idx = base + tid;
            int32_t x = 0;
            int nch = 0;
            if (idx < T) {
                x = rle_delta(st.nb + idx - 1, sh.lst[3 + idx], sh.lst[2 + idx], sh.lst[1 + idx], sh.lst[idx]);
                nch = rle_nchars(x);
            }
            int incl = nch;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            if (lane == 63) sh.stot[w] = (uint32_t)incl;
            __syncthreads();
            const uint32_t s0 = sh.stot[0], s1 = sh.stot[1], s2 = sh.stot[2], s3 = sh.stot[3];
            const uint32_t woff = (w > 0 ? s0 : 0) + (w > 1 ? s1 : 0) + (w > 2 ? s2 : 0);
            if (WRITE && idx < T) rle_emit(x, out, out_base + st.nchars + woff + (uint32_t)(incl - nch), out_end);
            st.nchars += s0 + s1 + s2 + s3;
            __syncthreads();                                    // stot is rewritten by the next round
        }
        const uint32_t n1 = sh.lst[T + 2], n2 = sh.lst[T + 1], n3 = sh.lst[T];
        st.b1 = n1; st.b2 = n2; st.b3 = n3;
        st.nb += T;
        __syncthreads();                                        // lst is rewritten by the next chunk
    }
}

// the last run ends at H*W; sizes (measure pass) = {number of runs, number of characters}
template <bool WRITE>
__device__ __forceinline__ void rle_finish(RleState& st, uint32_t HW, int k, int64_t* __restrict__ sizes, uint8_t* __restrict__ out, int64_t out_base,
                                           int64_t out_end) {
    if (threadIdx.x != 0) return;
    const int32_t x = rle_delta(st.nb - 1, HW, st.b1, st.b2, st.b3);
    if (WRITE) {
        rle_emit(x, out, out_base + st.nchars, out_end);
    } else {
        sizes[k * 2 + 0] = st.nb;
        sizes[k * 2 + 1] = st.nchars + rle_nchars(x);
    }
}

// measure pass (chars == NULL): sizes; write pass: offsets and a capacity
bool rle_buffers_ok(const int64_t* sizes, const int64_t* offsets, const uint8_t* chars, int64_t chars_capacity) {
    return chars ? (offsets && chars_capacity > 0) : sizes != nullptr;
}

}  // namespace
