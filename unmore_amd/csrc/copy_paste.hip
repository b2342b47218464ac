// Copy-paste augmentation of the detector's training batches (cad/engine/train_loop.py:90-248, CustomSimpleTrainer.copy_and_paste),
// a whole batch of independent (labeled, unlabeled) pairs per call.  Every pair has its own sizes and counts: the kernels walk a
// device table of umr_cp_pair entries (include/umr.h), blockIdx.y (overlap, decide: blockIdx.x) = the pair.
//
// Five launches, no atomics, no flags between workgroups; every mask lives as a bit set, 64 pixels of a row per word, rows padded to
// whole words (WW = ceil(Wu / 64) words per row), mask-major: [n_copy pasted | Nu existing | alpha][Hu][WW] per pair.
//   cp_pack_kernel     one wave per word position (row y, word wx) of the unlabeled frame, a lane per pixel.  The lane forms the two
//                      bilinear taps per axis of its pixel in the resized labeled frame ONCE and, per chosen mask, emits one bit: set iff
//                      a tap with a non-zero weight is set (what F.interpolate(...).bool() keeps).  __ballot makes the word.  The
//                      existing masks are packed by the same wave.
//   cp_overlap_kernel  one workgroup per tile of 8 pasted x 8 existing masks: the pasted words of a chunk are staged in LDS, a wave
//                      takes two existing masks, a lane ANDs an existing word with the 8 staged ones: __popcll into integer
//                      accumulators, one shuffle reduction per pair at the end.  Existing areas come from the same words.
//   cp_decide_kernel   keep copied instance i iff for every existing j: area_j > 0 and 2 * inter_ij < area_j -- the reference's float32
//                      inter / area < 0.5 (both integers are exact in float32 below 2^24 pixels, and 0 / 0 = NaN rejects every copy).
//   cp_compose_kernel  one wave per word position again: alpha = OR of the kept pasted words; the image byte is the resized labeled
//                      pixel under alpha (sampled here, only where it is needed: the resized image is never stored) and the unlabeled
//                      one elsewhere; existing masks & ~alpha and the kept pasted masks go out as bytes.
//   cp_stats_kernel    one workgroup per output mask: area and tight box (row and column extents of its words), or, for a pair
//                      whose unlabeled image had no instance, the reference's scaled and (swapped-) shifted float32 box.
//
// Resize arithmetic, float32, in this order (scale = in / out is formed on the host, in float32):
//   src = fmaf(scale, dst + 0.5, -0.5), clamped at 0;  i0 = min(floor(src), in - 1);  l = src - i0;  i1 = min(i0 + 1, in - 1)
//   value = (a * (1 - lx) + b * lx) * (1 - ly) + (c * (1 - lx) + d * lx) * ly, every product and sum rounded on its own.
// Contraction is off for the whole file: a mask bit depends on a weight being exactly zero, a byte on the rounding of each step.  The one
// fused multiply-add is written out, in the source index: torch's CPU kernels are built with FMA and form scale * (dst + 0.5) - 0.5 in
// one rounding, and the two forms disagree on WHETHER l == 0 (19 -> 95 pixels: scale = 0.2f, dst = 2 gives 0 with two roundings and
// 7.5e-9 fused), i.e. on mask bits.  With the fused index the bits equal F.interpolate(...).bool() in every case tried.
// Every load and store is guarded by the tables' own bounds (cp_load); the same input gives the same bytes on every run.
#pragma clang fp contract(off)
#include "umr_common.h"
#include <algorithm>

namespace {

constexpr int CP_THREADS = 256;
constexpr int OV_TP = 8, OV_TE = 8, OV_CH = 512;     // overlap tile: 8 pasted x 8 existing masks, 512 words of each per chunk (32 KiB LDS)

struct CpTotals {                                    // the extents of the shared buffers, the bounds every entry is checked against
    int64_t choice, words, inter, rows;
};

static_assert(sizeof(umr_cp_pair) == 152 && offsetof(umr_cp_pair, reserved) == 148, "umr_cp_pair is mirrored by _lib.CpPair");

struct CpPair {
    umr_cp_pair e;
    int WW;                                          // words per row
    int64_t nwm;                                     // words per mask
    bool ok;
};

__device__ __forceinline__ CpPair cp_load(const umr_cp_pair* __restrict__ pairs, int p, const CpTotals& T) {
    CpPair q;
    q.e = pairs[p];
    const umr_cp_pair& e = q.e;
    bool ok = e.Hl > 0 && e.Wl > 0 && e.Hu > 0 && e.Wu > 0 && e.Nl > 0 && e.Nu >= 0 && e.nc > 0 && e.nc <= e.Nl;
    ok = ok && (int64_t)e.Hu * e.Wu < ((int64_t)1 << 24) && (int64_t)e.Hl * e.Wl < ((int64_t)1 << 31);
    ok = ok && e.h_new > 0 && e.w_new > 0 && e.h_shift >= 0 && e.w_shift >= 0 && e.h_new <= e.Hu - e.h_shift && e.w_new <= e.Wu - e.w_shift;
    q.WW = ok ? (e.Wu + 63) >> 6 : 0;
    q.nwm = (int64_t)q.WW * (ok ? e.Hu : 0);
    ok = ok && e.word_off >= 0 && e.word_off <= T.words && ((int64_t)e.nc + e.Nu + 1) * q.nwm <= T.words - e.word_off;
    ok = ok && e.inter_off >= 0 && e.inter_off <= T.inter && ((int64_t)e.nc + 1) * e.Nu <= T.inter - e.inter_off;
    ok = ok && e.row_off >= 0 && e.row_off <= T.rows && (int64_t)e.nc + e.Nu <= T.rows - e.row_off;
    ok = ok && e.choice_off >= 0 && e.choice_off <= T.choice && e.nc <= T.choice - e.choice_off;
    ok = ok && e.l_image && e.l_masks && e.u_image && e.out_image && e.out_masks && (e.Nu == 0 || e.u_masks);
    q.ok = ok;
    return q;
}

struct CpTap {
    int i0, i1;
    float w0, w1;                                    // w1 = lambda, w0 = 1 - lambda
};

__device__ __forceinline__ CpTap cp_tap(int dst, int in, float scale) {
    float s = fmaf(scale, (float)dst + 0.5f, -0.5f);   // ONE rounding, on purpose: see the head of the file
    if (s < 0.f) s = 0.f;
    CpTap t;
    t.i0 = min((int)floorf(s), in - 1);
    float l = s - (float)t.i0;
    l = fminf(fmaxf(l, 0.f), 1.f);
    t.i1 = min(t.i0 + 1, in - 1);
    t.w1 = l;
    t.w0 = 1.f - l;
    return t;
}

__global__ __launch_bounds__(CP_THREADS) void cp_pack_kernel(const umr_cp_pair* __restrict__ pairs, const int32_t* __restrict__ choice,
                                                             CpTotals T, unsigned long long* __restrict__ words) {
    const int p = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const CpPair q = cp_load(pairs, p, T);
    if (!q.ok) return;
    const umr_cp_pair& e = q.e;
    unsigned long long* base = words + e.word_off;
    const int64_t plane_l = (int64_t)e.Hl * e.Wl;
    for (int64_t it = (int64_t)blockIdx.x * 4 + wv; it < q.nwm; it += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int y = (int)(it / q.WW), x = (int)(it % q.WW) * 64 + lane;
        const int py = y - e.h_shift, px = x - e.w_shift;
        const bool inx = x < e.Wu;
        const bool in = inx && py >= 0 && py < e.h_new && px >= 0 && px < e.w_new;
        CpTap ty = {0, 0, 1.f, 0.f}, tx = {0, 0, 1.f, 0.f};
        if (in) { ty = cp_tap(py, e.Hl, e.rh); tx = cp_tap(px, e.Wl, e.rw); }
        const int64_t o00 = (int64_t)ty.i0 * e.Wl + tx.i0, o01 = (int64_t)ty.i0 * e.Wl + tx.i1;
        const int64_t o10 = (int64_t)ty.i1 * e.Wl + tx.i0, o11 = (int64_t)ty.i1 * e.Wl + tx.i1;
        const bool ux = tx.w1 != 0.f, uy = ty.w1 != 0.f;
        for (int i = 0; i < e.nc; ++i) {
            const int c = choice[e.choice_off + i];
            bool bit = false;
            if (in && c >= 0 && c < e.Nl) {
                const uint8_t* m = e.l_masks + c * plane_l;
                bit = m[o00] != 0 || (ux && m[o01] != 0) || (uy && m[o10] != 0) || (ux && uy && m[o11] != 0);
            }
            const unsigned long long w = __ballot(bit);
            if (lane == 0) base[i * q.nwm + it] = w;
        }
        for (int j = 0; j < e.Nu; ++j) {
            const bool bit = inx && e.u_masks[((int64_t)j * e.Hu + y) * e.Wu + x] != 0;
            const unsigned long long w = __ballot(bit);
            if (lane == 0) base[(e.nc + j) * q.nwm + it] = w;
        }
    }
}

// inter: per pair [nc][Nu] intersections, then [Nu] existing areas
__global__ __launch_bounds__(CP_THREADS) void cp_overlap_kernel(const umr_cp_pair* __restrict__ pairs, CpTotals T,
                                                                const unsigned long long* __restrict__ words, int32_t* __restrict__ inter) {
    __shared__ unsigned long long dw[OV_TP][OV_CH];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CpPair q = cp_load(pairs, p, T);
    if (!q.ok || q.e.Nu == 0) return;
    const umr_cp_pair& e = q.e;
    const unsigned long long* base = words + e.word_off;
    int32_t* I = inter + e.inter_off;
    const int ntp = (e.nc + OV_TP - 1) / OV_TP, nte = (e.Nu + OV_TE - 1) / OV_TE;
    for (int64_t tile = blockIdx.y; tile < (int64_t)ntp * nte; tile += gridDim.y) {                // workgroup-uniform
        const int i0 = (int)(tile / nte) * OV_TP, j0 = (int)(tile % nte) * OV_TE;
        const int ci = min(OV_TP, e.nc - i0), cj = min(OV_TE, e.Nu - j0);
        int acc[OV_TE / 4][OV_TP], ar[OV_TE / 4];
#pragma unroll
        for (int jj = 0; jj < OV_TE / 4; ++jj) {
            ar[jj] = 0;
#pragma unroll
            for (int i = 0; i < OV_TP; ++i) acc[jj][i] = 0;
        }
        for (int64_t c0 = 0; c0 < q.nwm; c0 += OV_CH) {
            for (int idx = tid; idx < OV_TP * OV_CH; idx += CP_THREADS) {
                const int i = idx / OV_CH;
                const int64_t w = c0 + (idx % OV_CH);
                dw[i][idx % OV_CH] = (i < ci && w < q.nwm) ? base[(i0 + i) * q.nwm + w] : 0ull;
            }
            __syncthreads();
#pragma unroll
            for (int jj = 0; jj < OV_TE / 4; ++jj) {
                const int j = wv + jj * 4;
                if (j < cj) {                                                                       // wave-uniform
                    const unsigned long long* gw = base + (e.nc + j0 + j) * q.nwm;
                    for (int x = lane; x < OV_CH; x += 64) {
                        const int64_t w = c0 + x;
                        if (w >= q.nwm) break;
                        const unsigned long long g = gw[w];
                        if (!g) continue;
                        ar[jj] += __popcll(g);
#pragma unroll
                        for (int i = 0; i < OV_TP; ++i) acc[jj][i] += __popcll(g & dw[i][x]);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int jj = 0; jj < OV_TE / 4; ++jj) {
            const int j = wv + jj * 4;
            const int a = wave_sum(ar[jj]);
            if (lane == 0 && j < cj && i0 == 0) I[(int64_t)e.nc * e.Nu + j0 + j] = a;
#pragma unroll
            for (int i = 0; i < OV_TP; ++i) {
                const int v = wave_sum(acc[jj][i]);
                if (lane == 0 && j < cj && i < ci) I[(int64_t)(i0 + i) * e.Nu + j0 + j] = v;
            }
        }
    }
}

// stats: int32 [rows][2] = (flag, area).  A copied row's flag: kept or not; an existing row's flag: whether the pair keeps any copy
// (0 = the pair's output is the unlabeled item itself).
__global__ __launch_bounds__(CP_THREADS) void cp_decide_kernel(const umr_cp_pair* __restrict__ pairs, CpTotals T,
                                                               const int32_t* __restrict__ inter, int32_t* __restrict__ stats) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const CpPair q = cp_load(pairs, p, T);
    if (!q.ok) return;
    const umr_cp_pair& e = q.e;
    const int32_t* I = inter + e.inter_off;
    const int32_t* A = I + (int64_t)e.nc * e.Nu;
    int any = 0;
    for (int i = tid; i < e.nc; i += CP_THREADS) {
        int keep = 1;
        for (int j = 0; j < e.Nu; ++j) {
            const int64_t a = A[j], v = I[(int64_t)i * e.Nu + j];
            if (a <= 0 || 2 * v >= a) { keep = 0; break; }
        }
        stats[(e.row_off + e.Nu + i) * 2] = keep;
        any |= keep;
    }
    any = __syncthreads_or(any);
    for (int j = tid; j < e.Nu; j += CP_THREADS) stats[(e.row_off + j) * 2] = any ? 1 : 0;
}

__device__ __forceinline__ uint8_t cp_sample(const uint8_t* __restrict__ pl, int Wl, const CpTap& ty, const CpTap& tx) {
    const float a = (float)pl[(int64_t)ty.i0 * Wl + tx.i0], b = (float)pl[(int64_t)ty.i0 * Wl + tx.i1];
    const float c = (float)pl[(int64_t)ty.i1 * Wl + tx.i0], d = (float)pl[(int64_t)ty.i1 * Wl + tx.i1];
    const float top = a * tx.w0 + b * tx.w1, bot = c * tx.w0 + d * tx.w1;
    const float v = top * ty.w0 + bot * ty.w1;
    return (uint8_t)min(max((int)v, 0), 255);        // .byte(): truncation; the value never leaves [0, 255]
}

__global__ __launch_bounds__(CP_THREADS) void cp_compose_kernel(const umr_cp_pair* __restrict__ pairs, CpTotals T,
                                                                const int32_t* __restrict__ stats, unsigned long long* __restrict__ words) {
    const int p = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const CpPair q = cp_load(pairs, p, T);
    if (!q.ok) return;
    const umr_cp_pair& e = q.e;
    unsigned long long* base = words + e.word_off;
    unsigned long long* alpha_w = base + ((int64_t)e.nc + e.Nu) * q.nwm;
    const int32_t* keep = stats + (e.row_off + e.Nu) * 2;
    int any = 0;
    for (int i = 0; i < e.nc; ++i) any |= keep[i * 2];                                           // workgroup-uniform
    if (!any) return;
    const int64_t plane_l = (int64_t)e.Hl * e.Wl, plane_u = (int64_t)e.Hu * e.Wu;
    for (int64_t it = (int64_t)blockIdx.x * 4 + wv; it < q.nwm; it += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int y = (int)(it / q.WW), x = (int)(it % q.WW) * 64 + lane;
        const bool inx = x < e.Wu;
        unsigned long long alpha = 0;
        for (int i = 0; i < e.nc; ++i)
            if (keep[i * 2]) alpha |= base[i * q.nwm + it];
        if (lane == 0) alpha_w[it] = alpha;
        const bool on = (alpha >> lane) & 1ull;
        const int64_t o = (int64_t)y * e.Wu + x;
        if (inx) {
            if (on) {                                 // a set bit lies inside the pasted frame: pack wrote it from there
                const CpTap ty = cp_tap(y - e.h_shift, e.Hl, e.rh), tx = cp_tap(x - e.w_shift, e.Wl, e.rw);
#pragma unroll
                for (int c = 0; c < 3; ++c) e.out_image[c * plane_u + o] = cp_sample(e.l_image + c * plane_l, e.Wl, ty, tx);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) e.out_image[c * plane_u + o] = e.u_image[c * plane_u + o];
            }
            for (int j = 0; j < e.Nu; ++j)
                e.out_masks[j * plane_u + o] = (uint8_t)(((base[(e.nc + j) * q.nwm + it] & ~alpha) >> lane) & 1ull);
            for (int i = 0; i < e.nc; ++i)
                if (keep[i * 2]) e.out_masks[(e.Nu + i) * plane_u + o] = (uint8_t)((base[i * q.nwm + it] >> lane) & 1ull);
        }
    }
}

// boxes: float [rows][4]
__global__ __launch_bounds__(CP_THREADS) void cp_stats_kernel(const umr_cp_pair* __restrict__ pairs, const int32_t* __restrict__ choice,
                                                              CpTotals T, const unsigned long long* __restrict__ words,
                                                              int32_t* __restrict__ stats, float* __restrict__ boxes) {
    __shared__ int s_a[4], s_x0[4], s_x1[4], s_y0[4], s_y1[4];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CpPair q = cp_load(pairs, p, T);
    if (!q.ok) return;
    const umr_cp_pair& e = q.e;
    for (int m = blockIdx.x; m < e.Nu + e.nc; m += gridDim.x) {                                  // workgroup-uniform
        const int64_t row = e.row_off + m;
        if (!stats[row * 2]) continue;                // a copy that is not kept, or a pair that keeps none
        const bool existing = m < e.Nu;
        const unsigned long long* base = words + e.word_off;
        const unsigned long long* mw = base + (existing ? (int64_t)e.nc + m : (int64_t)m - e.Nu) * q.nwm;
        const unsigned long long* alpha_w = base + ((int64_t)e.nc + e.Nu) * q.nwm;
        int a = 0, x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
        for (int64_t it = tid; it < q.nwm; it += CP_THREADS) {
            unsigned long long w = mw[it];
            if (existing) w &= ~alpha_w[it];
            if (w) {
                const int y = (int)(it / q.WW), xb = (int)(it % q.WW) * 64;
                a += __popcll(w);
                x0 = min(x0, xb + __ffsll((long long)w) - 1);
                x1 = max(x1, xb + 63 - __clzll((long long)w));
                y0 = min(y0, y);
                y1 = max(y1, y);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            x0 = min(x0, __shfl_xor(x0, o, 64)); x1 = max(x1, __shfl_xor(x1, o, 64));
            y0 = min(y0, __shfl_xor(y0, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
        }
        __syncthreads();                              // the previous mask's sums have been read
        if (lane == 0) { s_a[wv] = a; s_x0[wv] = x0; s_x1[wv] = x1; s_y0[wv] = y0; s_y1[wv] = y1; }
        __syncthreads();
        if (tid == 0) {
            a = s_a[0] + s_a[1] + s_a[2] + s_a[3];
            x0 = min(min(s_x0[0], s_x0[1]), min(s_x0[2], s_x0[3])); x1 = max(max(s_x1[0], s_x1[1]), max(s_x1[2], s_x1[3]));
            y0 = min(min(s_y0[0], s_y0[1]), min(s_y0[2], s_y0[3])); y1 = max(max(s_y1[0], s_y1[1]), max(s_y1[2], s_y1[3]));
            stats[row * 2 + 1] = a;
            float* b = boxes + row * 4;
            if (e.Nu > 0) {                           // BitMasks.get_bounding_boxes: [x_min, y_min, x_max + 1, y_max + 1], zeros when empty
                b[0] = a ? (float)x0 : 0.f; b[1] = a ? (float)y0 : 0.f;
                b[2] = a ? (float)(x1 + 1) : 0.f; b[3] = a ? (float)(y1 + 1) : 0.f;
            } else {                                  // train_loop.py:173-174,191-194: scaled, then x += h_shift and y += w_shift (sic)
                const int c = choice[e.choice_off + m];
                const bool cok = c >= 0 && c < e.Nl && e.l_boxes;
                const float* s = e.l_boxes + (int64_t)(cok ? c : 0) * 4;
                const float fh = (float)e.h_shift, fw = (float)e.w_shift;
                b[0] = cok ? s[0] * e.sx + fh : 0.f; b[1] = cok ? s[1] * e.sy + fw : 0.f;
                b[2] = cok ? s[2] * e.sx + fh : 0.f; b[3] = cok ? s[3] * e.sy + fw : 0.f;
            }
        }
    }
}

}  // namespace

extern "C" int64_t umr_copy_paste_workspace(int64_t total_words, int64_t total_inter) {
    if (total_words < 0 || total_inter < 0) return 0;
    return total_words * 8 + ((total_inter + 1) / 2) * 8;
}

extern "C" int umr_copy_paste(const umr_cp_pair* pairs, int P, const int32_t* choice, int64_t total_choice, int64_t total_words,
                              int64_t total_inter, int64_t total_rows, int64_t max_words_per_mask, int max_nc, int max_nu, int phases,
                              int32_t* stats, float* boxes, void* workspace, int64_t workspace_bytes, umr_stream_t stream) {
    UMR_CHECK_ARG(P >= 0 && total_choice >= 0 && total_words >= 0 && total_inter >= 0 && total_rows >= 0, "copy_paste: negative extent");
    UMR_CHECK_ARG(max_words_per_mask >= 0 && max_nc >= 0 && max_nu >= 0, "copy_paste: negative maximum");
    UMR_CHECK_ARG(phases > 0 && phases < 8, "copy_paste: phases is a mask of 1 (pack), 2 (overlap, decide), 4 (compose, stats)");
    if (P == 0) return UMR_OK;
    UMR_CHECK_ARG(pairs && choice && stats && boxes && workspace, "copy_paste: null pointer");
    UMR_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "copy_paste: workspace not 8-byte aligned");
    UMR_CHECK_ARG(workspace_bytes >= umr_copy_paste_workspace(total_words, total_inter), "copy_paste: workspace too small");
    UMR_CHECK_ARG(P <= 65535, "copy_paste: more than 65535 pairs");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* words = (unsigned long long*)workspace;
    int32_t* inter = (int32_t*)(words + total_words);
    const CpTotals T = {total_choice, total_words, total_inter, total_rows};
    const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>((max_words_per_mask + 3) / 4, 1), 2048);
    if (phases & 1) {
        cp_pack_kernel<<<dim3(gx, P), CP_THREADS, 0, s>>>(pairs, choice, T, words);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        if (max_nu > 0) {
            const int64_t tiles = (int64_t)((max_nc + OV_TP - 1) / OV_TP) * ((max_nu + OV_TE - 1) / OV_TE);
            cp_overlap_kernel<<<dim3(P, (unsigned)std::min<int64_t>(std::max<int64_t>(tiles, 1), 256)), CP_THREADS, 0, s>>>(pairs, T, words, inter);
            UMR_LAUNCH_CHECK();
        }
        cp_decide_kernel<<<P, CP_THREADS, 0, s>>>(pairs, T, inter, stats);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 4) {
        cp_compose_kernel<<<dim3(gx, P), CP_THREADS, 0, s>>>(pairs, T, stats, words);
        UMR_LAUNCH_CHECK();
        const unsigned gm = (unsigned)std::min<int64_t>(std::max<int64_t>((int64_t)max_nc + max_nu, 1), 1024);
        cp_stats_kernel<<<dim3(gm, P), CP_THREADS, 0, s>>>(pairs, choice, T, words, stats, boxes);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
