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
// Back end (rle_stream.h, shared with poly_rle.hip), per chunk of 2048 stream positions (wave w owns 512 consecutive ones; lane l takes w*512 + e*64 + l, e < 8, so that a
// wave's 64 LDS byte reads are consecutive): flag the positions whose pixel differs from its predecessor's (the pixel before position 0
// is 0), rank the flags in stream order (ballots inside a wave, four wave totals through LDS), put their positions -- the run
// BOUNDARIES -- into an LDS list behind the last three boundaries of earlier chunks; then one thread per boundary closes a run: its
// length, the delta against the run two back, its character count; a second scan gives the character offsets; the characters are
// written.  Run order, offsets and bytes are functions of the input alone: the same input gives the same bytes on every run.
#include "umr_common.h"
#include "mask_paste.h"
#include "rle_stream.h"

namespace {

constexpr int RLE_TILE_BYTES = 128 * 1024;     // LDS for the transposed strip (the back end's list and totals are static, ~8 KiB)

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
