// The detector's input path (cad/data/dataset_mapper.py:152-213 with ResizeShortestEdge + RandomFlip, cad/data/transforms/transform.py:
// 94-163, and GeneralizedRCNN.preprocess_image, cad/modeling/meta_arch/rcnn.py:229-240): three kernels, each ONE launch for a whole ragged
// batch, driven by int64 descriptors and int32 tables that the host builds in float64 and uploads in one buffer
// (unmore_amd/detector_input.py).  Everything here is integer arithmetic or one float32 subtract and one float32 divide: the bytes equal
// PIL's and torch's.
//
//   di_bilinear_kernel   PIL's Image.resize(BILINEAR) on 8-bit RGB: two separable passes, horizontal first, the intermediate rounded
//                        and clipped to a byte.  A workgroup owns an output tile of TH rows x TW columns (all three channels); it runs
//                        the horizontal pass for exactly the input rows the tile's vertical taps read, into LDS as bytes, then the
//                        vertical pass out of LDS: the intermediate never touches memory.  Reads HWC, writes planar CHW, the flip is
//                        applied at the store.  Per output index the tables give (lo, n) and n fixed-point weights k (22 fractional
//                        bits, non-negative, summing to about 2^22: an int32 accumulator cannot overflow);
//                        byte = clip((2^21 + sum_j in[lo + j] * k_j) >> 22).  An axis that keeps its size gets the table lo = i, n = 1,
//                        k = 2^22, which returns the byte itself: no second rounding, PIL's skipped pass.
//                        Extreme ratios: the host SHRINKS THE TILE, there is no two-launch form.  TW = 64 and TH is the largest of
//                        32, 16, ..., 1 whose staged rows fit DI_LDS_PIX = 10880 staged pixels (x 3 channels = 32640 bytes of LDS);
//                        when even one output row does not fit (a vertical scale beyond about 84), TW halves down to 1, which holds
//                        10880 input rows.  A 4000 -> 240 side has 35-tap rows: TH = 8.  A tile whose rows do not fit is skipped.
//   di_nearest_kernel    PIL's Image.resize(NEAREST) of every instance mask: a gather through the two index tables (the host forms
//                        them by repeated addition, as PIL does), flip at the store, 0 / 1 bytes out (a bool tensor).  A workgroup
//                        owns a band of rows of one mask, ORs what it wrote and sets the mask's non-empty flag with one integer
//                        atomicOr -- the only atomic here, and the result does not depend on arrival order.
//   di_normalize_kernel  (float32(u8) - mean[c]) / std[c], an IEEE divide, into [B,3,Hp,Wp] float32 with the padding value around:
//                        every float of the output is written, no memset; 16 bytes per store whenever Wp is a multiple of 4 (any
//                        size_divisibility that is), one float per store otherwise.  Pure streaming.
//
// Every table offset and every index read from a table is checked against the extents the call passes; a descriptor that breaks them
// is skipped.  The same input gives the same bytes on every run.
#pragma clang fp contract(off)
#include "umr_common.h"
#include <algorithm>

namespace {

constexpr int DI_THREADS = 256;
constexpr int DI_LDS_PIX = 10880;                    // staged pixels per tile (x 3 channels): detector_input.LDS_PIX mirrors it
constexpr int DI_MAX_TW = 64;
constexpr int BL_DESC = 16, NN_DESC = 13, NP_DESC = 4;
constexpr int DI_PREC = 22;
constexpr int NN_BAND = 4096;                        // output pixels per workgroup of the nearest kernel (rounded up to 4 k whole rows)

// bilinear descriptor, int64 [B][16]:
//  0 src (u8 [H,W,3])  1 dst (u8 [3,nh,nw])  2 H  3 W  4 nh  5 nw  6 flip (1 horizontal, 2 vertical)
//  7 hb: offset of the horizontal (lo, n) pairs [nw][2] in tab   8 hk: of the weights [nw][hks]   9 hks
// 10 vb  11 vk  12 vks (the same for the vertical axis, [nh])   13 TH  14 TW  15 first tile of the image in the grid
__device__ __forceinline__ int di_find(const int64_t* __restrict__ desc, int B, int stride, int field, int64_t blk) {
    int lo = 0, hi = B - 1;                          // the last image whose first block is <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * stride + field] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool di_slice_ok(int64_t off, int64_t len, int64_t total) {
    return off >= 0 && len >= 0 && off <= total && len <= total - off;
}

__global__ __launch_bounds__(DI_THREADS) void di_bilinear_kernel(const int64_t* __restrict__ desc, int B, const int32_t* __restrict__ tab,
                                                                 int64_t tab_len) {
    __shared__ uint8_t s[DI_LDS_PIX * 3];
    const int tid = threadIdx.x;
    const int img = di_find(desc, B, BL_DESC, 15, blockIdx.x);
    const int64_t* d = desc + (int64_t)img * BL_DESC;
    const uint8_t* __restrict__ src = (const uint8_t*)(uintptr_t)d[0];
    uint8_t* __restrict__ dst = (uint8_t*)(uintptr_t)d[1];
    const int64_t H = d[2], W = d[3], nh = d[4], nw = d[5];
    const int flip = (int)d[6];
    const int64_t hb = d[7], hk = d[8], hks = d[9], vb = d[10], vk = d[11], vks = d[12];
    const int64_t TH = d[13], TW = d[14];
    const int64_t lim = (int64_t)1 << 30;
    bool ok = src && dst && H > 0 && W > 0 && nh > 0 && nw > 0 && H < lim && W < lim && nh < lim && nw < lim && H * W < lim && nh * nw < lim;
    ok = ok && TH >= 1 && TW >= 1 && TW <= DI_MAX_TW && TH <= DI_LDS_PIX && hks >= 1 && vks >= 1 && hks < lim && vks < lim;
    ok = ok && di_slice_ok(hb, 2 * nw, tab_len) && di_slice_ok(hk, nw * hks, tab_len);
    ok = ok && di_slice_ok(vb, 2 * nh, tab_len) && di_slice_ok(vk, nh * vks, tab_len);
    if (!ok) return;                                                                             // workgroup-uniform
    const int tiles_x = (int)((nw + TW - 1) / TW), tiles_y = (int)((nh + TH - 1) / TH);
    const int64_t t = (int64_t)blockIdx.x - d[15];
    if (t < 0 || t >= (int64_t)tiles_x * tiles_y) return;
    const int y0 = (int)(t / tiles_x) * (int)TH, x0 = (int)(t % tiles_x) * (int)TW;
    const int th = (int)std::min<int64_t>(TH, nh - y0), tw = (int)std::min<int64_t>(TW, nw - x0);
    // the input rows the tile's vertical taps read: lo and lo + n do not decrease with the output index
    const int32_t* vbt = tab + vb;
    const int r0 = std::min<int>(std::max<int>(vbt[2 * y0], 0), (int)H);
    const int r1 = std::min<int>(std::max<int>(vbt[2 * (y0 + th - 1)] + vbt[2 * (y0 + th - 1) + 1], r0), (int)H);
    const int R = r1 - r0;
    if ((int64_t)R * TW > DI_LDS_PIX) return;                                                    // the host sized the tile so that it fits
    // ---- horizontal pass: staged[c][r][x], bytes
    const int32_t* hbt = tab + hb;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);                   // a wave per staged row: no division per element
    const int ne = tw * 3;
    for (int r = wv; r < R; r += DI_THREADS / 64) {
        const uint8_t* row = src + ((int64_t)(r0 + r) * W) * 3;
        for (int e = lane; e < ne; e += 64) {
            const int x = e / 3, c = e - x * 3;
            const int lo = hbt[2 * (x0 + x)];
            const int n = std::min<int>(hbt[2 * (x0 + x) + 1], (int)hks);
            const int32_t* k = tab + hk + (int64_t)(x0 + x) * hks;
            int acc = 1 << (DI_PREC - 1);
            for (int j = 0; j < n; ++j) {
                const int xi = lo + j;
                if (xi >= 0 && xi < W) acc += (int)row[(int64_t)xi * 3 + c] * k[j];
            }
            s[(c * R + r) * (int)TW + x] = (uint8_t)std::min(std::max(acc >> DI_PREC, 0), 255);
        }
    }
    __syncthreads();
    // ---- vertical pass out of LDS, flip at the store
    const int64_t plane = nh * nw;
    for (int q = wv; q < th * 3; q += DI_THREADS / 64) {                                        // a wave per output row of a channel
        const int c = q / th, y = q - c * th;
        const int lo = vbt[2 * (y0 + y)];
        const int n = std::min<int>(vbt[2 * (y0 + y) + 1], (int)vks);
        const int32_t* k = tab + vk + (int64_t)(y0 + y) * vks;
        const int64_t oy = (flip & 2) ? nh - 1 - (y0 + y) : y0 + y;
        for (int x = lane; x < tw; x += 64) {
            int acc = 1 << (DI_PREC - 1);
            for (int j = 0; j < n; ++j) {
                const int r = lo + j - r0;
                if (r >= 0 && r < R) acc += (int)s[(c * R + r) * (int)TW + x] * k[j];
            }
            const int64_t ox = (flip & 1) ? nw - 1 - (x0 + x) : x0 + x;
            dst[c * plane + oy * nw + ox] = (uint8_t)std::min(std::max(acc >> DI_PREC, 0), 255);
        }
    }
}

// nearest descriptor, int64 [B][13]:
//  0 src (u8 / bool, mask n at src + n * stride)  1 dst (u8 [N,nh,nw])  2 N  3 H  4 W  5 nh  6 nw  7 flip  8 tx: offset of the column
//  table [nw] in tab  9 ty: of the row table [nh]  10 first flag of the image  11 first workgroup of the image in the grid
//  12 stride: bytes from one input mask to the next (>= H * W; rle.decode starts every mask on a 16-byte boundary)
__global__ __launch_bounds__(DI_THREADS) void di_nearest_kernel(const int64_t* __restrict__ desc, int B, const int32_t* __restrict__ tab,
                                                                int64_t tab_len, int32_t* __restrict__ flags, int64_t n_flags) {
    const int tid = threadIdx.x;
    const int img = di_find(desc, B, NN_DESC, 11, blockIdx.x);
    const int64_t* d = desc + (int64_t)img * NN_DESC;
    const uint8_t* __restrict__ src = (const uint8_t*)(uintptr_t)d[0];
    uint8_t* __restrict__ dst = (uint8_t*)(uintptr_t)d[1];
    const int64_t N = d[2], H = d[3], W = d[4], nh = d[5], nw = d[6];
    const int flip = (int)d[7];
    const int64_t tx = d[8], ty = d[9], flag0 = d[10], stride = d[12];
    const int64_t lim = (int64_t)1 << 30;
    bool ok = src && dst && N > 0 && H > 0 && W > 0 && nh > 0 && nw > 0 && H * W < lim && nh * nw < lim && H < lim && W < lim && nh < lim &&
              nw < lim && N < lim && stride >= H * W;
    ok = ok && di_slice_ok(tx, nw, tab_len) && di_slice_ok(ty, nh, tab_len) && di_slice_ok(flag0, N, n_flags);
    if (!ok) return;                                                                             // workgroup-uniform
    const int rows = (int)(((NN_BAND + nw - 1) / nw + 3) / 4 * 4);                                // rows per band: a multiple of the 4 waves
    const int bands = (int)((nh + rows - 1) / rows);
    const int64_t t = (int64_t)blockIdx.x - d[11];
    if (t < 0 || t >= N * bands) return;
    const int64_t n = t / bands;
    const int y0 = (int)(t % bands) * rows;
    const int th = (int)std::min<int64_t>(rows, nh - y0);
    const uint8_t* m = src + n * stride;
    uint8_t* o = dst + n * nh * nw;
    const int32_t* txt = tab + tx;
    const int32_t* tyt = tab + ty;
    int any = 0;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);                   // a wave per output row
    for (int r = wv; r < th; r += DI_THREADS / 64) {
        const int y = y0 + r, sy = tyt[y];
        const bool row_ok = sy >= 0 && sy < H;
        const uint8_t* mr = m + (int64_t)(row_ok ? sy : 0) * W;
        uint8_t* orow = o + ((flip & 2) ? nh - 1 - y : (int64_t)y) * nw;
        for (int x = lane; x < nw; x += 64) {
            const int sx = txt[x];
            uint8_t v = 0;
            if (row_ok && sx >= 0 && sx < W) v = mr[sx] != 0;
            any |= v;
            orow[(flip & 1) ? nw - 1 - x : (int64_t)x] = v;
        }
    }
    any = __syncthreads_or(any);
    if (tid == 0 && any) atomicOr(&flags[flag0 + n], 1);
}

// normalise descriptor, int64 [B][4]: 0 src (u8 [3,h,w])  1 h  2 w  3 unused
struct DiNorm {
    float mean[3], std[3], pad;
};

__global__ __launch_bounds__(DI_THREADS) void di_normalize_kernel(const int64_t* __restrict__ desc, int B, int Hp, int Wp, DiNorm P,
                                                                  float* __restrict__ out) {
    const int64_t rows = (int64_t)B * 3 * Hp;                                                    // a workgroup per output row, grid-strided
    const bool vec = (Wp & 3) == 0;                                                              // every row then starts on 16 bytes
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int y = (int)(r % Hp);
        const int64_t q = r / Hp;
        const int c = (int)(q % 3), b = (int)(q / 3);
        const int64_t* d = desc + (int64_t)b * NP_DESC;
        const uint8_t* src = (const uint8_t*)(uintptr_t)d[0];
        const int64_t h = d[1], w = d[2];
        const bool in_row = src && h > 0 && w > 0 && y < h;
        const uint8_t* p = src + (in_row ? (c * h + y) * w : 0);
        const float mean = c == 0 ? P.mean[0] : c == 1 ? P.mean[1] : P.mean[2], sd = c == 0 ? P.std[0] : c == 1 ? P.std[1] : P.std[2];
        float* orow = out + r * Wp;
        if (vec) {
            for (int x = (int)threadIdx.x * 4; x < Wp; x += DI_THREADS * 4) {
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (in_row && x + i < w) ? ((float)p[x + i] - mean) / sd : P.pad;
                *reinterpret_cast<float4*>(orow + x) = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
            for (int x = threadIdx.x; x < Wp; x += DI_THREADS) orow[x] = (in_row && x < w) ? ((float)p[x] - mean) / sd : P.pad;
        }
    }
}

}  // namespace

extern "C" int umr_det_resize_bilinear(const int64_t* desc, int B, const int32_t* tab, int64_t tab_len, int64_t total_tiles,
                                       umr_stream_t stream) {
    UMR_CHECK_ARG(B >= 0 && tab_len >= 0 && total_tiles >= 0, "det_resize_bilinear: negative extent");
    if (B == 0 || total_tiles == 0) return UMR_OK;
    UMR_CHECK_ARG(desc && tab, "det_resize_bilinear: null pointer");
    UMR_CHECK_ARG(total_tiles < ((int64_t)1 << 31), "det_resize_bilinear: more than 2^31 tiles");
    di_bilinear_kernel<<<(unsigned)total_tiles, DI_THREADS, 0, (hipStream_t)stream>>>(desc, B, tab, tab_len);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_det_resize_nearest(const int64_t* desc, int B, const int32_t* tab, int64_t tab_len, int64_t total_blocks, int32_t* flags,
                                      int64_t n_flags, umr_stream_t stream) {
    UMR_CHECK_ARG(B >= 0 && tab_len >= 0 && total_blocks >= 0 && n_flags >= 0, "det_resize_nearest: negative extent");
    if (B == 0 || total_blocks == 0) return UMR_OK;
    UMR_CHECK_ARG(desc && tab && flags, "det_resize_nearest: null pointer");
    UMR_CHECK_ARG(total_blocks < ((int64_t)1 << 31), "det_resize_nearest: more than 2^31 workgroups");
    di_nearest_kernel<<<(unsigned)total_blocks, DI_THREADS, 0, (hipStream_t)stream>>>(desc, B, tab, tab_len, flags, n_flags);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_det_normalize_pad(const int64_t* desc, int B, int Hp, int Wp, float mean0, float mean1, float mean2, float std0,
                                     float std1, float std2, float pad_value, float* out, umr_stream_t stream) {
    UMR_CHECK_ARG(B >= 0 && Hp >= 0 && Wp >= 0, "det_normalize_pad: negative extent");
    const int64_t total = (int64_t)B * 3 * Hp * Wp;
    if (total == 0) return UMR_OK;
    UMR_CHECK_ARG(desc && out, "det_normalize_pad: null pointer");
    UMR_CHECK_ARG(((uintptr_t)out & 15) == 0, "det_normalize_pad: out not 16-byte aligned");
    const DiNorm P = {{mean0, mean1, mean2}, {std0, std1, std2}, pad_value};
    const unsigned grid = (unsigned)std::min<int64_t>((int64_t)B * 3 * Hp, 8192);
    di_normalize_kernel<<<grid, DI_THREADS, 0, (hipStream_t)stream>>>(desc, B, Hp, Wp, P, out);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
