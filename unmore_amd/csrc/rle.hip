// COCO run-length encoding (pycocotools' maskApi.c string format) of binary masks on the device -- the `segmentation` field of the
// records object scoring writes (object_scoring.py:166-170,257-272).  Pixels are taken in COLUMN-major order (j = x*H + y); `counts`
// are the lengths of the alternating runs starting with zeros; run i is written as the signed value counts[i] - (i > 2 ? counts[i-2]
// : 0) in 5-bit groups, low group first, 0x20 = "another group follows", each group as the character group + 48.
//
// Two producers of a pixel stream share one back end (one workgroup of 256 threads per mask, no scratch memory, no atomics):
//   * rle_encode_tile_kernel / rle_encode_linear_kernel: a mask [H,W] u8 that is already in memory.  Row-major memory, column-major
//     order: a strip of TW whole columns is read row by row (coalesced) and written TRANSPOSED into LDS, then streamed from there.
//   * mask_paste_rle_kernel: the pasted union mask of a proposal, evaluated pixel by pixel from the two crop masks in LDS with the
//     paste_axis / paste_bit of mask_paste.h (the instructions umr_mask_paste runs) -- over the box's columns only; the mask itself is
//     never written.
// Back end, per chunk of 2048 stream positions (wave w owns 512 consecutive ones; lane l takes w*512 + e*64 + l, e < 8, so that a
// wave's 64 LDS byte reads are consecutive): flag the positions whose pixel differs from its predecessor's (the pixel before position 0
// is 0), rank the flags in stream order (ballots inside a wave, four wave totals through LDS), put their positions -- the run
// BOUNDARIES -- into an LDS list behind the last three boundaries of earlier chunks; then one thread per boundary closes a run: its
// length, the delta against the run two back, its character count; a second scan gives the character offsets; the characters are
// written.  Run order, offsets and bytes are functions of the input alone: the same input gives the same bytes on every run.
#include "umr_common.h"
#include "mask_paste.h"

namespace {

constexpr int RLE_THREADS = 256, RLE_E = 8, RLE_WAVE_SPAN = 64 * RLE_E, RLE_CHUNK = RLE_THREADS * RLE_E;
constexpr int RLE_TILE_BYTES = 128 * 1024;     // LDS for the transposed strip (the back end's list and totals are static, ~8 KiB)

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

// ---- a mask in memory, H == 1 or W == 1: column-major order is memory order
struct LinearProducer {
    const uint8_t* m;
    __device__ __forceinline__ int value(uint32_t p) const { return m[p] != 0; }
    __device__ __forceinline__ int before() const { return 0; }
    __device__ __forceinline__ uint32_t gpos(uint32_t p) const { return p; }
};
template <bool WRITE>
__global__ __launch_bounds__(RLE_THREADS) void rle_encode_linear_kernel(const uint8_t* __restrict__ masks, uint32_t HW, int64_t* __restrict__ sizes,
                                                                        const int64_t* __restrict__ offsets, uint8_t* __restrict__ chars, int64_t cap) {
    __shared__ RleShared sh;
    const int k = blockIdx.x;
    RleState st;
    const LinearProducer prod{masks + (int64_t)k * HW};
    const int64_t ob = WRITE ? offsets[k] : 0;
    rle_stream<WRITE>(prod, HW, sh, st, chars, ob, cap);
    rle_finish<WRITE>(st, HW, k, sizes, chars, ob, cap);
}

// ---- a mask in memory, general: strips of TW whole columns through a transposed LDS tile.  Column c of the strip is the HP bytes at
// c * HP; HP = H rounded up to a multiple of 4 with HP / 4 odd, so that the 32 lanes of a store group, which write one row of 32
// neighbouring columns (strips of 32 columns or more, byte path), fall on 32 different banks; the dword path stores a row of 16 x 4
// columns per 16 lanes, two lanes to a bank, which a store does not pay for.
struct TileProducer {
    const uint8_t* tile;
    uint32_t H, HP, strip_pos;        // strip_pos: column-major position of the strip's first pixel
    float inv_h;
    int prev;                         // the pixel before the strip (last row of the column to its left)
    __device__ __forceinline__ int value(uint32_t p) const {
        uint32_t c = (uint32_t)((float)p * inv_h);                  // p < 2^17: exact in f32, the quotient is off by one at the most
        if (c * H > p) --c;
        if ((c + 1) * H <= p) ++c;
        return tile[c * HP + (p - c * H)];
    }
    __device__ __forceinline__ int before() const { return prev; }
    __device__ __forceinline__ uint32_t gpos(uint32_t p) const { return strip_pos + p; }
};
template <bool WRITE, bool DWORDS>
__global__ __launch_bounds__(RLE_THREADS) void rle_encode_tile_kernel(const uint8_t* __restrict__ masks, int H, int W, int HP, int TW, int tw_shift,
                                                                      int64_t* __restrict__ sizes, const int64_t* __restrict__ offsets,
                                                                      uint8_t* __restrict__ chars, int64_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
    __shared__ RleShared sh;
    const int k = blockIdx.x, tid = threadIdx.x;
    const uint8_t* m = masks + (int64_t)k * H * W;
    RleState st;
    const int64_t ob = WRITE ? offsets[k] : 0;
    for (int x0 = 0; x0 < W; x0 += TW) {
        const int tw = min(TW, W - x0);
        if (DWORDS) {           // W % 4 == 0 and a 4-byte aligned base: one dword = one row of four neighbouring columns
            const int qs = tw_shift - 2, nq = tw >> 2;
            for (int i = tid; i < (H << qs); i += RLE_THREADS) {
                const int y = i >> qs, q = i & ((1 << qs) - 1);
                if (q < nq) {
                    const uint32_t v = *(const uint32_t*)(m + (int64_t)y * W + x0 + q * 4);
                    unsigned char* d = tile + (q * 4) * HP + y;
                    d[0] = (v & 0xffu) != 0; d[HP] = (v & 0xff00u) != 0; d[2 * HP] = (v & 0xff0000u) != 0; d[3 * HP] = (v & 0xff000000u) != 0;
                }
            }
        } else {
            for (int i = tid; i < (H << tw_shift); i += RLE_THREADS) {
                const int y = i >> tw_shift, c = i & (TW - 1);
                if (c < tw) tile[c * HP + y] = m[(int64_t)y * W + x0 + c] != 0;
            }
        }
        __syncthreads();
        const TileProducer prod{tile, (uint32_t)H, (uint32_t)HP, (uint32_t)x0 * (uint32_t)H, 1.0f / (float)H, x0 > 0 ? (m[(int64_t)(H - 1) * W + x0 - 1] != 0) : 0};
        rle_stream<WRITE>(prod, (uint32_t)tw * (uint32_t)H, sh, st, chars, ob, cap);
        __syncthreads();                                        // the tile is refilled by the next strip
    }
    rle_finish<WRITE>(st, (uint32_t)H * (uint32_t)W, k, sizes, chars, ob, cap);
}

// ---- the pasted union mask of a proposal, never written.  The stream is the box's columns (the part of the box inside the image), top
// to bottom; when that part is lower than the image every column gets one more position below its last row (value 0: the first of the
// zeros up to the next column's first row), so that a pixel's predecessor in the stream has the value of its predecessor in the image's
// column-major order.  A part as high as the image has no such position between its columns (they adjoin in the image's order too), and
// gets one after its last column when that is not the image's last: the first zero to the right of the box.
struct PasteProducer {
    const unsigned char *mc, *mb;
    int S, ox, oy, hb, wb;            // ox, oy: the visible part's corner relative to the box's; hb, wb: the BOX's size (the resize's output size)
    int vx, vy, vh, vw;               // the visible part's corner in the image, its height and width
    uint32_t H, hl;                   // hl = vh + (vh < H): positions per column
    __device__ __forceinline__ int value(uint32_t p) const {
        const uint32_t cx = p / hl, cy = p - cx * hl;
        if ((int)cy >= vh || (int)cx >= vw) return 0;
        const PasteAxis ay = paste_axis(oy + (int)cy, hb, S), ax = paste_axis(ox + (int)cx, wb, S);
        return (paste_bit(mc, S, ay, ax) || paste_bit(mb, S, ay, ax)) ? 1 : 0;
    }
    __device__ __forceinline__ int before() const { return 0; }
    __device__ __forceinline__ uint32_t gpos(uint32_t p) const {
        const uint32_t cx = p / hl, cy = p - cx * hl;
        return ((uint32_t)vx + cx) * H + (uint32_t)vy + cy;
    }
};
template <bool WRITE>
__global__ __launch_bounds__(RLE_THREADS) void mask_paste_rle_kernel(const float* __restrict__ sdf, const float* __restrict__ center,
                                                                     const int32_t* __restrict__ boxes, const int64_t* __restrict__ select, int S, int H, int W,
                                                                     int64_t* __restrict__ sizes, const int64_t* __restrict__ offsets,
                                                                     uint8_t* __restrict__ chars, int64_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ RleShared sh;
    const int k = blockIdx.x;
    const int b = (int)select[k];
    unsigned char* mc = lds;
    unsigned char* mb = lds + S * S;
    float mn = 0.f, ms = 0.f;
    paste_masks_to_lds(sdf, center, b, S, mc, mb, mn, ms);
    __syncthreads();
    const int x1 = boxes[b * 4 + 0], y1 = boxes[b * 4 + 1], x2 = boxes[b * 4 + 2], y2 = boxes[b * 4 + 3];
    const int hb = y2 - y1, wb = x2 - x1;
    // mask_paste_kernel sets a pixel of the image iff it lies in the box: the part of the box inside the image
    const int vx = max(x1, 0), vy = max(y1, 0), vw = min(x2, W) - vx, vh = min(y2, H) - vy;
    RleState st;
    const int64_t ob = WRITE ? offsets[k] : 0;
    if (hb > 0 && wb > 0 && vw > 0 && vh > 0) {
        const uint32_t hl = (uint32_t)vh + (vh < H ? 1u : 0u);
        const PasteProducer prod{mc, mb, S, vx - x1, vy - y1, hb, wb, vx, vy, vh, vw, (uint32_t)H, hl};
        uint32_t n = hl * (uint32_t)vw;
        if (vh == H && vx + vw < W) ++n;                           // the first zero right of a part as high as the image
        if (vh < H && vy + vh == H && vx + vw == W) --n;           // the position below the image's last pixel is the end, not a pixel
        rle_stream<WRITE>(prod, n, sh, st, chars, ob, cap);
    }
    rle_finish<WRITE>(st, (uint32_t)H * (uint32_t)W, k, sizes, chars, ob, cap);
}

// measure pass (chars == NULL): sizes; write pass: offsets and a capacity
bool rle_buffers_ok(const int64_t* sizes, const int64_t* offsets, const uint8_t* chars, int64_t chars_capacity) {
    return chars ? (offsets && chars_capacity > 0) : sizes != nullptr;
}

}  // namespace

extern "C" int umr_rle_encode(const uint8_t* masks, int K, int H, int W, int64_t* sizes, const int64_t* offsets, uint8_t* chars,
                              int64_t chars_capacity, umr_stream_t stream) {
    UMR_CHECK_ARG(masks && K > 0 && H > 0 && W > 0, "rle_encode: bad arguments");
    UMR_CHECK_ARG((int64_t)H * W < ((int64_t)1 << 31), "rle_encode: H * W must be below 2^31");
    UMR_CHECK_ARG(rle_buffers_ok(sizes, offsets, chars, chars_capacity),
                  "rle_encode: the measure pass needs sizes; the write pass needs offsets, chars and a positive chars_capacity");
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    hipStream_t s = (hipStream_t)stream;
    if (H == 1 || W == 1) {
        if (chars) hipLaunchKernelGGL(rle_encode_linear_kernel<true>, dim3(K), dim3(RLE_THREADS), 0, s, masks, HW, sizes, offsets, chars, chars_capacity);
        else hipLaunchKernelGGL(rle_encode_linear_kernel<false>, dim3(K), dim3(RLE_THREADS), 0, s, masks, HW, sizes, offsets, chars, chars_capacity);
        UMR_LAUNCH_CHECK();
        return UMR_OK;
    }
    int HP = (H + 3) & ~3;
    if (((HP >> 2) & 1) == 0) HP += 4;
    int tw_shift = 10;                                           // up to 1024 columns per strip, fewer for a tall or a narrow image
    while (tw_shift > 2 && ((int64_t)HP << tw_shift) > RLE_TILE_BYTES) --tw_shift;
    if (((int64_t)HP << tw_shift) > RLE_TILE_BYTES)
        return umr_set_error(UMR_ERR_UNSUPPORTED, "rle_encode: a mask with more than one column is limited to 32764 rows (four whole columns in LDS)");
    while (tw_shift > 2 && (1 << (tw_shift - 1)) >= W) --tw_shift;
    const int TW = 1 << tw_shift;
    const size_t lds = (size_t)HP << tw_shift;
    const bool dwords = (W & 3) == 0 && ((uintptr_t)masks & 3) == 0;
#define UMR_RLE_TILE_LAUNCH(WR, DW)                                                                                                   \
    do {                                                                                                                              \
        UMR_SET_MAX_LDS_ONCE((rle_encode_tile_kernel<WR, DW>), RLE_TILE_BYTES);                                                       \
        hipLaunchKernelGGL((rle_encode_tile_kernel<WR, DW>), dim3(K), dim3(RLE_THREADS), lds, s, masks, H, W, HP, TW, tw_shift, sizes, \
                           offsets, chars, chars_capacity);                                                                           \
    } while (0)
    if (chars) { if (dwords) UMR_RLE_TILE_LAUNCH(true, true); else UMR_RLE_TILE_LAUNCH(true, false); }
    else { if (dwords) UMR_RLE_TILE_LAUNCH(false, true); else UMR_RLE_TILE_LAUNCH(false, false); }
#undef UMR_RLE_TILE_LAUNCH
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_mask_paste_rle(const float* sdf_maps, const float* center_fields, const int32_t* boxes, const int64_t* select, int K, int S,
                                  int H, int W, int64_t* sizes, const int64_t* offsets, uint8_t* chars, int64_t chars_capacity,
                                  umr_stream_t stream) {
    UMR_CHECK_ARG(sdf_maps && center_fields && boxes && select && K > 0 && S > 0 && H > 0 && W > 0, "mask_paste_rle: bad arguments");
    UMR_CHECK_ARG((int64_t)H * W < ((int64_t)1 << 31), "mask_paste_rle: H * W must be below 2^31");
    UMR_CHECK_ARG(rle_buffers_ok(sizes, offsets, chars, chars_capacity),
                  "mask_paste_rle: the measure pass needs sizes; the write pass needs offsets, chars and a positive chars_capacity");
    if ((int64_t)S * S * 2 > 128 * 1024) return umr_set_error(UMR_ERR_UNSUPPORTED, "mask_paste_rle: crop larger than the LDS mask planes (S <= 256)");
    const size_t lds = (size_t)S * S * 2;
    hipStream_t s = (hipStream_t)stream;
    if (chars) {
        UMR_SET_MAX_LDS_ONCE(mask_paste_rle_kernel<true>, 128 * 1024);
        hipLaunchKernelGGL(mask_paste_rle_kernel<true>, dim3(K), dim3(RLE_THREADS), lds, s, sdf_maps, center_fields, boxes, select, S, H, W, sizes, offsets,
                           chars, chars_capacity);
    } else {
        UMR_SET_MAX_LDS_ONCE(mask_paste_rle_kernel<false>, 128 * 1024);
        hipLaunchKernelGGL(mask_paste_rle_kernel<false>, dim3(K), dim3(RLE_THREADS), lds, s, sdf_maps, center_fields, boxes, select, S, H, W, sizes, offsets,
                           chars, chars_capacity);
    }
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
