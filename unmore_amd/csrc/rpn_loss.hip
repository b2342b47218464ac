// The training half of the stage-3 detector's RPN (cad/modeling/meta_arch/rcnn.py:165, 333: self.proposal_generator(images, features,
// gt_instances), which is Detectron2's RPN.label_and_sample_anchors and RPN.losses): every anchor of every image is matched to the
// image's ground truths and labelled, a batch of anchors per image is sampled, and the objectness and localisation losses over the
// sampled anchors are formed with their gradients.  The anchors are rebuilt from (level, y, x, a) as rpn.hip does; no anchor tensor
// and no [G, R] matrix exists, the head's outputs are read in place, nothing is read back, and there are no float atomics (integer
// atomics form row maxima on the bits of non-negative floats and counts: integer max and sum have no order), so the same input
// gives the same bytes.  The level descriptors travel in the kernels' arguments.
//
// Anchor r: level after level, inside a level f = (y * W + x) * A + a; r = (the levels before) + f.  R anchors per image.
//   rl_match_kernel    a thread per (anchor, image); the image's ground truths pass through LDS in tiles of 256 with their areas.
//                      Per anchor the maximum IoU and the FIRST index that reaches it (`>`, torch's CPU max(dim=0)); per ground truth the
//                      maximum over the anchors: atomicMax on the float's bits, in LDS per workgroup, then one per tile entry to memory.
//                      A ground truth with a non-finite coordinate takes no part and is counted (`bad`).
//   rl_label_kernel    label = v < lo ? 0 : (v < hi ? -1 : 1) (all 0 in an image without usable ground truths); with low-quality
//                      matches an anchor becomes 1 if for some ground truth g its IoU -- RECOMPUTED by the same inline function, so the
//                      same bits -- equals row g's maximum (the matched index is not changed; a ground truth that overlaps no anchor has
//                      row maximum 0 and marks every anchor of IoU 0 with it: Detectron2's behaviour); then the boundary filter, label
//                      -1 unless x1 >= -t, y1 >= -t, x2 < w + t, y2 < h + t (t < 0: off).  int8 labels, and the counts P of 1s and Q of 0s.
//   rl_part_kernel     only when R > RL_SELECT_SHARE: one workgroup per (part of 16384 anchors, class, image) leaves the part's own best
//                      (up to the class's share of the batch), in r order, in the workspace; the parts lie one after the other, so their
//                      concatenation is again in r order (rpn.hip's two-step select).
//   rl_select_kernel   one workgroup per (class, image): num_pos = min(P, pos_cap), num_neg = min(Q, B - num_pos); the num_pos (num_neg)
//                      anchors of label 1 (0) with the LARGEST key, equal keys to the lower r, by select_in_order.h's four-pass radix
//                      select over the image's anchors or over the parts' survivors; they are written in ascending r: index[n, 0 ..
//                      num_pos) the positives, [num_pos, num_pos + num_neg) the negatives, with the matched ground truth of each.
//   rl_loss_kernel     one workgroup per image, a thread per sample (strided): its logit and, for a positive, its four deltas from the
//                      head's layout, widened; the terms in float64; the gradients by plain stores into maps the caller zeroed (the
//                      positions are distinct).  The per-thread sums go through block_sum_fixed: one partial per image.
//   rl_finish_kernel   the partials in index order; the two losses as float32.
//
// Key of anchor r of image n (31 bits): keys[n, r] & 0x7fffffff when keys are given, else with s_lo / s_hi the low / high 32 bits of seed
//   fmix(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16          (murmur3's 32-bit finaliser, mod 2^32)
//   key = fmix(fmix(r ^ s_lo) ^ (n * 0x9e3779b9 + s_hi)) >> 1                                    (det_box.h's sample_key)
// Arithmetic.  Matching and labelling: float32, no contraction, every operation rounded on its own:
//   anchor      sx = float(x * stride) + off, sy = float(y * stride) + off (off = offset * stride, exact); (sx + c0, sy + c1, sx + c2, sy + c3)
//   iou(a, b)   = inter > 0 ? inter / ((area_a + area_b) - inter) : 0, det_box.h's box_iou_match, the division correctly rounded
// Losses: float64 on the float32 anchors, ground truths and widened predictions (at most B samples per image; with smooth_l1_beta > 0
// the gradient (p - t) / beta would otherwise carry t's float32 rounding relative to a difference that can be small):
//   cls         max(x, 0) - x t + log1p(exp(-|x|)); d/dx = t ? -1 / (1 + exp(x)) : 1 / (1 + exp(-x))   (sigmoid(x) - t without cancellation)
//   get         dx = wx * (tcx - scx) / sw; dw = ww * log(tw / sw)   (Box2BoxTransform.get_deltas in box_loss.hip's order)
//   smooth-L1   e = p - t; beta < 1e-5: |e|, sign(e) (0 at 0); |e| < beta: .5 e^2 / beta, e / beta; else |e| - .5 beta, sign(e)
//   both sums times their scale = loss_weight / (B * N); the gradients times the same scale, rounded once to the inputs' type.
#pragma clang fp contract(off)
#include "umr_common.h"
#include "det_box.h"
#include "select_in_order.h"
#include <algorithm>
#include <float.h>
#include <limits.h>

namespace {

constexpr int RL_MAX_LEVELS = 8;
constexpr int RL_MAX_BATCH = 1024;
constexpr int RL_THREADS = 256;
constexpr int RL_GT_TILE = 256;                       // == RL_THREADS: one load per thread
constexpr int RL_SELECT_THREADS = 1024;
constexpr int RL_SELECT_SHARE = 16384;                // anchors per workgroup of rl_part_kernel
constexpr int RL_PART_THREADS = 256;
constexpr int RL_COUNTERS = 5;                        // P, Q, sampled positives, sampled negatives, bad ground truths

struct RlLevel {
    const void* logits;               // [N,A,H,W]       (the loss only)
    const void* deltas;               // [N,4A,H,W]
    void* g_logits;                   // the gradient maps, same shapes and type
    void* g_deltas;
    int H, W, stride;
    int n;                            // H * W * A
    int first;                        // the sum of n over the levels before
    float off;                        // offset * stride
};

struct RlPlan {
    RlLevel lv[RL_MAX_LEVELS];
    int L, N, A, R;
};

using Partial = SumPartial<2, 1>;     // per image: the objectness and the localisation sum; the samples

struct RlAt { int l, a, pix; };       // where anchor r sits: level, cell anchor, y * W + x

__device__ __forceinline__ RlAt rl_locate(const RlPlan& pl, int r) {
    int l = 0;
    while (l + 1 < pl.L && r >= pl.lv[l + 1].first) ++l;
    const int f = r - pl.lv[l].first, pix = f / pl.A;
    return RlAt{l, f - pix * pl.A, pix};
}

__device__ __forceinline__ void rl_anchor(const RlPlan& pl, const float* __restrict__ cells, const RlAt at, float b[4]) {
    const RlLevel& lv = pl.lv[at.l];
    const int y = at.pix / lv.W, x = at.pix - y * lv.W;
    grid_anchor(cells + (at.l * GRID_MAX_A + at.a) * 4, x, y, lv.stride, lv.off, b);
}

// the image's ground truths [g_lo, g_lo + G), trusted only as far as the table is ordered
__device__ __forceinline__ void rl_gt_range(const int32_t* __restrict__ gt_first, int n, int n_gt, int& g_lo, int& G) {
    g_lo = gt_first[n];
    const int g_hi = gt_first[n + 1];
    if (g_lo < 0 || g_hi < g_lo || g_hi > n_gt) { g_lo = 0; G = 0; } else { G = g_hi - g_lo; }
}

// ---------------------------------------------------------------------------------------------------------------- match
__global__ __launch_bounds__(RL_THREADS) void rl_match_kernel(RlPlan pl, const float* __restrict__ cells, const float* __restrict__ gt_boxes,
                                                              const int32_t* __restrict__ gt_first, int n_gt, float* __restrict__ mval,
                                                              int32_t* __restrict__ midx, unsigned* __restrict__ row_max,
                                                              int32_t* __restrict__ counters) {
    __shared__ float gt[RL_GT_TILE][5];                                   // x1 y1 x2 y2 area
    __shared__ int ok[RL_GT_TILE];
    __shared__ unsigned smax[RL_GT_TILE];
    __shared__ int s_bad;
    const int tid = threadIdx.x, n = blockIdx.y, r = blockIdx.x * RL_THREADS + tid;
    const bool live = r < pl.R;
    int g_lo, G;
    rl_gt_range(gt_first, n, n_gt, g_lo, G);
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) rl_anchor(pl, cells, rl_locate(pl, r), p);
    const float p_area = box_area(p[0], p[1], p[2], p[3]);
    if (tid == 0) s_bad = 0;
    float best = -1.f;
    int best_g = 0;
    for (int g0 = 0; g0 < G; g0 += RL_GT_TILE) {
        const int cnt = min(RL_GT_TILE, G - g0);
        __syncthreads();
        if (tid < cnt) {
            const float* b = gt_boxes + (int64_t)(g_lo + g0 + tid) * 4;
            const bool fin = box_finite(b[0]) && box_finite(b[1]) && box_finite(b[2]) && box_finite(b[3]);
            gt[tid][0] = b[0]; gt[tid][1] = b[1]; gt[tid][2] = b[2]; gt[tid][3] = b[3];
            gt[tid][4] = box_area(b[0], b[1], b[2], b[3]);
            ok[tid] = fin;
            smax[tid] = 0u;
            if (!fin) atomicAdd(&s_bad, 1);
        }
        __syncthreads();
        if (live) {
            for (int g = 0; g < cnt; ++g) {
                if (!ok[g]) continue;
                const float v = box_iou_match(gt[g][0], gt[g][1], gt[g][2], gt[g][3], gt[g][4], p[0], p[1], p[2], p[3], p_area);
                if (v > best) { best = v; best_g = g0 + g; }              // strict: the first index that reaches the maximum
                if (v > 0.f) {
                    const unsigned bits = __float_as_uint(v);             // v > 0: the bits order as the values do
                    if (bits > ((volatile unsigned*)smax)[g]) atomicMax(&smax[g], bits);
                }
            }
        }
        __syncthreads();
        if (tid < cnt && smax[tid] > 0u) atomicMax(row_max + g_lo + g0 + tid, smax[tid]);
    }
    if (live) {
        mval[(int64_t)n * pl.R + r] = best > 0.f ? best : 0.f;
        midx[(int64_t)n * pl.R + r] = best_g;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) counters[n * RL_COUNTERS + 4] = s_bad;
}

// ---------------------------------------------------------------------------------------------------------------- label
__global__ __launch_bounds__(RL_THREADS) void rl_label_kernel(RlPlan pl, const float* __restrict__ cells, const float* __restrict__ image_sizes,
                                                              const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_first,
                                                              int n_gt, const float* __restrict__ mval, const unsigned* __restrict__ row_max,
                                                              float lo, float hi, int low_quality, float boundary,
                                                              int8_t* __restrict__ labels, int32_t* __restrict__ counters) {
    __shared__ float gt[RL_GT_TILE][6];                                   // x1 y1 x2 y2 area, the row's maximum
    __shared__ int ok[RL_GT_TILE];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, n = blockIdx.y, r = blockIdx.x * RL_THREADS + tid;
    const bool live = r < pl.R;
    int g_lo, G;
    rl_gt_range(gt_first, n, n_gt, g_lo, G);
    const int usable = G - counters[n * RL_COUNTERS + 4];                 // the match launch left the number of bad ground truths there
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) rl_anchor(pl, cells, rl_locate(pl, r), p);
    const float p_area = box_area(p[0], p[1], p[2], p[3]);
    if (tid < 2) s_cnt[tid] = 0;
    int label = 0;
    if (live && usable > 0) {
        const float v = mval[(int64_t)n * pl.R + r];
        label = v < lo ? 0 : (v < hi ? -1 : 1);
    }
    if (low_quality && usable > 0) {
        for (int g0 = 0; g0 < G; g0 += RL_GT_TILE) {
            const int cnt = min(RL_GT_TILE, G - g0);
            __syncthreads();
            if (tid < cnt) {
                const float* b = gt_boxes + (int64_t)(g_lo + g0 + tid) * 4;
                gt[tid][0] = b[0]; gt[tid][1] = b[1]; gt[tid][2] = b[2]; gt[tid][3] = b[3];
                gt[tid][4] = box_area(b[0], b[1], b[2], b[3]);
                gt[tid][5] = __uint_as_float(row_max[g_lo + g0 + tid]);
                ok[tid] = box_finite(b[0]) && box_finite(b[1]) && box_finite(b[2]) && box_finite(b[3]);
            }
            __syncthreads();
            if (live && label != 1) {
                for (int g = 0; g < cnt; ++g) {
                    if (!ok[g]) continue;
                    const float v = box_iou_match(gt[g][0], gt[g][1], gt[g][2], gt[g][3], gt[g][4], p[0], p[1], p[2], p[3], p_area);
                    if (v == gt[g][5]) { label = 1; break; }
                }
            }
        }
    }
    if (live && boundary >= 0.f) {
        const float h = image_sizes[n * 2], w = image_sizes[n * 2 + 1];
        const bool inside = p[0] >= -boundary && p[1] >= -boundary && p[2] < w + boundary && p[3] < h + boundary;
        if (!inside) label = -1;
    }
    if (live) labels[(int64_t)n * pl.R + r] = (int8_t)label;
    const unsigned long long v1 = __ballot(live && label == 1), v0 = __ballot(live && label == 0);
    __syncthreads();
    if ((tid & 63) == 0) {
        if (v1) atomicAdd(&s_cnt[0], __popcll(v1));
        if (v0) atomicAdd(&s_cnt[1], __popcll(v0));
    }
    __syncthreads();
    if (tid < 2 && s_cnt[tid]) atomicAdd(counters + n * RL_COUNTERS + tid, s_cnt[tid]);
}

// ---------------------------------------------------------------------------------------------------------------- select
// the keys of one image's anchors (rows: labels, keys and the hash's mix of that image): 0 for an anchor of another label, else the
// 31-bit key with the top bit set
struct RlKeys {
    const int8_t* labels; const int32_t* keys; int want; unsigned s_lo, mix;
    __device__ __forceinline__ unsigned of(int r) const {
        const unsigned k = keys ? (unsigned)keys[r] : sample_key_mixed((unsigned)r, s_lo, mix);
        return (k & 0x7fffffffu) | 0x80000000u;
    }
    __device__ __forceinline__ unsigned key(int64_t r) const { return labels[r] == want ? of((int)r) : 0u; }
};

// the anchors [r0, r0 + ...) of the image: one part
struct RlPartKeys {
    RlKeys k; int r0;
    __device__ __forceinline__ unsigned key(int64_t i) const { return k.key(r0 + i); }
};

// the parts' survivors one after the other, k slots per part (at a pitch of B), -1 in a slot that is not used
struct RlSurvivorKeys {
    RlKeys k; const int32_t* surv; int per, B, R;
    __device__ __forceinline__ int anchor(int64_t i) const {
        const int p = (int)(i / per), j = (int)(i - (int64_t)p * per);
        return surv[(int64_t)p * B + j];
    }
    __device__ __forceinline__ unsigned key(int64_t i) const {
        const int r = anchor(i);
        return (r >= 0 && r < R) ? k.of(r) : 0u;
    }
};

struct RlQuota { int k, base, want; };

// the class's share of the batch from the label launch's counts P and Q
__device__ __forceinline__ RlQuota rl_quota(const int32_t* counters, int n, int cls, int R, int B, int pos_cap) {
    const int P = min(max(counters[n * RL_COUNTERS], 0), R), Q = min(max(counters[n * RL_COUNTERS + 1], 0), R);
    const int num_pos = min(P, pos_cap), num_neg = min(Q, B - num_pos);
    return cls == 0 ? RlQuota{num_pos, 0, 1} : RlQuota{num_neg, num_pos, 0};
}

// only for R > RL_SELECT_SHARE: one workgroup per (part, class, image) leaves the part's k best, in r order, in surv [N,2,parts,B]
__global__ __launch_bounds__(RL_PART_THREADS) void rl_part_kernel(RlPlan pl, const int8_t* __restrict__ labels, const int32_t* __restrict__ keys,
                                                                  unsigned s_lo, unsigned s_hi, int B, int pos_cap,
                                                                  const int32_t* __restrict__ counters, int32_t* surv, int parts) {
    __shared__ int hist[256];
    __shared__ int wtot[32];
    const int part = blockIdx.x, cls = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const RlQuota q = rl_quota(counters, n, cls, pl.R, B, pos_cap);
    const int r0 = part * RL_SELECT_SHARE;
    if (q.k <= 0 || part >= parts || r0 >= pl.R) return;                   // workgroup-uniform
    const int64_t row = (int64_t)n * pl.R;
    const RlPartKeys src{RlKeys{labels + row, keys ? keys + row : nullptr, q.want, s_lo, sample_mix((unsigned)n, s_hi)}, r0};
    int32_t* out = surv + (((int64_t)n * 2 + cls) * parts + part) * B;
    const int c = select_in_order(src, (int64_t)min(RL_SELECT_SHARE, pl.R - r0), q.k, hist, wtot, SelectStoreIndex{out});
    for (int j = tid; j < q.k; j += RL_PART_THREADS) out[j] = j < c ? out[j] + r0 : -1;
}

__global__ __launch_bounds__(RL_SELECT_THREADS) void rl_select_kernel(RlPlan pl, const int8_t* __restrict__ labels,
                                                                      const int32_t* __restrict__ midx, const int32_t* __restrict__ keys,
                                                                      unsigned s_lo, unsigned s_hi, int B, int pos_cap,
                                                                      const int32_t* __restrict__ surv, int parts,
                                                                      int32_t* __restrict__ index, int32_t* __restrict__ sample_gt,
                                                                      int32_t* __restrict__ counts, int8_t* __restrict__ dense,
                                                                      int32_t* counters) {
    __shared__ int hist[256];
    __shared__ int wtot[32];
    __shared__ int32_t picked[RL_MAX_BATCH];
    const int cls = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const RlQuota q = rl_quota(counters, n, cls, pl.R, B, pos_cap);
    const int64_t row = (int64_t)n * pl.R;
    if (q.k > 0) {                                                        // workgroup-uniform
        const RlKeys keys_of{labels + row, keys ? keys + row : nullptr, q.want, s_lo, sample_mix((unsigned)n, s_hi)};
        const RlSurvivorKeys from{keys_of, surv + ((int64_t)n * 2 + cls) * parts * B, q.k, B, pl.R};
        const int c = parts <= 1 ? select_in_order(keys_of, (int64_t)pl.R, q.k, hist, wtot, SelectStoreIndex{picked})
                                 : select_in_order(from, (int64_t)parts * q.k, q.k, hist, wtot, SelectStoreIndex{picked});
        for (int j = tid; j < min(c, q.k); j += RL_SELECT_THREADS) {
            int r = parts <= 1 ? picked[j] : from.anchor(picked[j]);
            if (r < 0 || r >= pl.R) r = 0;                                // never: the indices are this call's own
            index[(int64_t)n * B + q.base + j] = r;
            sample_gt[(int64_t)n * B + q.base + j] = midx[row + r];
            if (dense) dense[row + r] = (int8_t)q.want;
        }
    }
    __syncthreads();                                                      // every thread has read the counts before they change
    if (tid == 0) {
        counts[n * 2 + cls] = q.k;
        counters[n * RL_COUNTERS + 2 + cls] = q.k;
    }
}

// ---------------------------------------------------------------------------------------------------------------- losses
__device__ __forceinline__ double rl_load(const void* p, int dtype, int64_t at) {
    return dtype == UMR_BF16 ? (double)(float)((const bf16_t*)p)[at] : (double)((const float*)p)[at];
}
__device__ __forceinline__ void rl_store(void* p, int dtype, int64_t at, double v) {
    if (dtype == UMR_BF16) ((bf16_t*)p)[at] = (bf16_t)(float)v; else ((float*)p)[at] = (float)v;
}

__global__ __launch_bounds__(RL_THREADS) void rl_loss_kernel(RlPlan pl, int dtype, const float* __restrict__ cells,
                                                             const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_first,
                                                             int n_gt, const int32_t* __restrict__ index, const int32_t* __restrict__ sample_gt,
                                                             const int32_t* __restrict__ counts, int B, double wx, double wy, double ww,
                                                             double wh, double beta, double scale_cls, double scale_loc,
                                                             Partial* __restrict__ partials) {
    __shared__ double red_d[8];
    __shared__ long long red_n[4];
    const int tid = threadIdx.x, n = blockIdx.x;
    const int n_pos = min(max(counts[n * 2], 0), B), n_all = n_pos + min(max(counts[n * 2 + 1], 0), B - n_pos);
    int g_lo, G;
    rl_gt_range(gt_first, n, n_gt, g_lo, G);
    double sums[2] = {0.0, 0.0};
    long long cnt[1] = {0};
    const double wk[4] = {wx, wy, ww, wh};
    for (int s = tid; s < n_all; s += RL_THREADS) {
        const int r = index[(int64_t)n * B + s];
        if (r < 0 || r >= pl.R) continue;                                 // never for samples this library wrote
        const RlAt at = rl_locate(pl, r);
        const RlLevel& lv = pl.lv[at.l];
        const int64_t HW = (int64_t)lv.H * lv.W;
        const bool pos = s < n_pos;
        const int64_t la = ((int64_t)n * pl.A + at.a) * HW + at.pix;
        const double x = rl_load(lv.logits, dtype, la);
        sums[0] += ((x > 0.0 ? x : 0.0) - (pos ? x : 0.0)) + log1p(exp(-fabs(x)));
        rl_store(lv.g_logits, dtype, la, (pos ? -1.0 / (1.0 + exp(x)) : 1.0 / (1.0 + exp(-x))) * scale_cls);
        cnt[0] += 1;
        if (!pos) continue;
        const int gi = sample_gt[(int64_t)n * B + s];
        if (gi < 0 || gi >= G) continue;                                  // likewise
        float a[4];
        rl_anchor(pl, cells, at, a);
        const float* tb = gt_boxes + (int64_t)(g_lo + gi) * 4;
        const double sw = (double)a[2] - a[0], sh = (double)a[3] - a[1];
        const double scx = a[0] + .5 * sw, scy = a[1] + .5 * sh;
        const double tw = (double)tb[2] - tb[0], th = (double)tb[3] - tb[1];
        const double tcx = tb[0] + .5 * tw, tcy = tb[1] + .5 * th;
        const double t[4] = {wk[0] * (tcx - scx) / sw, wk[1] * (tcy - scy) / sh, wk[2] * log(tw / sw), wk[3] * log(th / sh)};
        const int64_t da = ((int64_t)n * 4 * pl.A + at.a * 4) * HW + at.pix;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double e = rl_load(lv.deltas, dtype, da + c * HW) - t[c], m = fabs(e);
            double l, g;
            if (beta < 1e-5) {
                l = m;
                g = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
            } else if (m < beta) {
                l = .5 * e * e / beta;
                g = e / beta;
            } else {
                l = m - .5 * beta;
                g = e > 0.0 ? 1.0 : -1.0;
            }
            sums[1] += l;
            rl_store(lv.g_deltas, dtype, da + c * HW, g * scale_loc);
        }
    }
    block_sum_fixed(sums, cnt, red_d, red_n);
    if (tid == 0) {
        Partial q;
        q.d[0] = sums[0];
        q.d[1] = sums[1];
        q.c[0] = (int32_t)cnt[0];
        q.c[1] = 0;
        partials[n] = q;
    }
}

__global__ __launch_bounds__(RL_THREADS) void rl_finish_kernel(const Partial* __restrict__ partials, int n_partials, double scale_cls,
                                                               double scale_loc, float* __restrict__ losses) {
    __shared__ double red_d[8];
    __shared__ long long red_n[4];
    double d[2];
    long long n[1];
    partials_sum_fixed(partials, n_partials, d, n, red_d, red_n);
    if (threadIdx.x == 0) {
        losses[0] = (float)(d[0] * scale_cls);
        losses[1] = (float)(d[1] * scale_loc);
    }
}

// the plan of a call from the host array of levels (`per` int64 each); UMR_OK or the error set
int rl_plan(const int64_t* levels, int per, int n_levels, int64_t N, int A, double offset, RlPlan& pl) {
    UMR_CHECK_ARG(levels && n_levels >= 1 && n_levels <= RL_MAX_LEVELS, "rpn_loss: between 1 and 8 levels");
    UMR_CHECK_ARG(N >= 1 && N <= 65535, "rpn_loss: between 1 and 65535 images");
    UMR_CHECK_ARG(A >= 1 && A <= GRID_MAX_A, "rpn_loss: between 1 and 16 anchors per position");
    UMR_CHECK_ARG(offset >= 0.0 && offset < 1.0, "rpn_loss: offset must lie in [0, 1)");
    pl = RlPlan{};
    pl.L = n_levels; pl.N = (int)N; pl.A = A;
    int64_t R = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int64_t* e = levels + (int64_t)per * l;
        RlLevel& lv = pl.lv[l];
        UMR_CHECK_ARG(e[0] >= 1 && e[1] >= 1 && e[0] <= INT_MAX && e[1] <= INT_MAX && e[0] * e[1] <= INT_MAX / A - 1,
                      "rpn_loss: a level needs 0 < H * W * A < 2^31");
        UMR_CHECK_ARG(e[2] >= 1 && e[2] <= (1 << 24) && e[0] * e[2] <= (1 << 24) && e[1] * e[2] <= (1 << 24),
                      "rpn_loss: a stride must be positive with H * stride and W * stride at most 2^24");
        lv.H = (int)e[0]; lv.W = (int)e[1]; lv.stride = (int)e[2];
        lv.n = lv.H * lv.W * A;
        lv.first = (int)R;
        lv.off = (float)(offset * (double)lv.stride);                 // exact: the caller checks that the product is a float32 value
        if (per == 7) {
            UMR_CHECK_ARG(e[3] && e[4] && e[5] && e[6], "rpn_loss: a level without logits, deltas or gradient maps");
            lv.logits = (const void*)(uintptr_t)e[3];
            lv.deltas = (const void*)(uintptr_t)e[4];
            lv.g_logits = (void*)(uintptr_t)e[5];
            lv.g_deltas = (void*)(uintptr_t)e[6];
        }
        R += lv.n;
        UMR_CHECK_ARG(R < INT_MAX, "rpn_loss: 2^31 - 1 anchors per image or more");
    }
    pl.R = (int)R;
    return UMR_OK;
}

inline int rl_parts(int R) { return (R + RL_SELECT_SHARE - 1) / RL_SELECT_SHARE; }

}  // namespace

extern "C" int64_t umr_rpn_label_workspace(const int64_t* levels, int n_levels, int64_t N, int A, int batch_size) {
    RlPlan pl;
    if (rl_plan(levels, 3, n_levels, N, A, 0.0, pl) != UMR_OK || batch_size < 1 || batch_size > RL_MAX_BATCH) return -1;
    const int64_t parts = rl_parts(pl.R);
    return parts > 1 ? N * 2 * parts * batch_size * 4 : 0;
}

extern "C" int umr_rpn_label_sample(const int64_t* levels, int n_levels, int64_t N, int A, const float* cells, const float* image_sizes,
                                    const float* gt_boxes, const int32_t* gt_first, int64_t n_gt, float iou_lo, float iou_hi,
                                    int allow_low_quality, int batch_size, int pos_cap, float boundary_thresh, double offset, int64_t seed,
                                    const int32_t* keys, int phases, float* matched_vals, int32_t* matched_idxs, float* row_max,
                                    int8_t* labels, int32_t* sample_index, int32_t* sample_gt, int32_t* counts, int8_t* dense_labels,
                                    int32_t* counters, void* workspace, int64_t workspace_bytes, umr_stream_t stream) {
    RlPlan pl;
    if (int st = rl_plan(levels, 3, n_levels, N, A, offset, pl)) return st;
    const int parts = rl_parts(pl.R);
    UMR_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && (parts <= 1 || workspace_bytes >= (int64_t)N * 2 * parts * batch_size * 4),
                  "rpn_loss: workspace missing, too small or not 4-byte aligned");
    UMR_CHECK_ARG(cells && image_sizes && gt_first, "rpn_loss: the cell anchors [L,16,4], the image sizes [N,2] and gt_first [N+1] on the device");
    UMR_CHECK_ARG(n_gt >= 0 && n_gt < INT_MAX && (n_gt == 0 || gt_boxes), "rpn_loss: 0 <= n_gt < 2^31 - 1, and the boxes when there are any");
    UMR_CHECK_ARG(iou_lo == iou_lo && iou_hi == iou_hi && iou_lo <= iou_hi, "rpn_loss: the IoU thresholds must be ordered numbers");
    UMR_CHECK_ARG(batch_size >= 1 && batch_size <= RL_MAX_BATCH && pos_cap >= 0 && pos_cap <= batch_size,
                  "rpn_loss: 1 <= batch_size <= 1024 and 0 <= pos_cap <= batch_size");
    UMR_CHECK_ARG(boundary_thresh == boundary_thresh, "rpn_loss: the boundary threshold is NaN");
    UMR_CHECK_ARG(matched_vals && matched_idxs && row_max && labels && sample_index && sample_gt && counts && counters, "rpn_loss: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((pl.R + RL_THREADS - 1) / RL_THREADS, pl.N);
    const int ng = (int)n_gt;
    if (phases & 1) {
        if (hipMemsetAsync(counters, 0, (size_t)N * RL_COUNTERS * 4, s) != hipSuccess ||
            hipMemsetAsync(row_max, 0, (size_t)std::max<int64_t>(n_gt, 1) * 4, s) != hipSuccess)
            return umr_set_error(UMR_ERR_HIP, "rpn_loss: hipMemsetAsync failed");
        hipLaunchKernelGGL(rl_match_kernel, grid, dim3(RL_THREADS), 0, s, pl, cells, gt_boxes, gt_first, ng, matched_vals, matched_idxs,
                           (unsigned*)row_max, counters);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        hipLaunchKernelGGL(rl_label_kernel, grid, dim3(RL_THREADS), 0, s, pl, cells, image_sizes, gt_boxes, gt_first, ng, matched_vals,
                           (const unsigned*)row_max, iou_lo, iou_hi, allow_low_quality, boundary_thresh, labels, counters);
        UMR_LAUNCH_CHECK();
    }
    const unsigned s_lo = (unsigned)((uint64_t)seed & 0xffffffffu), s_hi = (unsigned)((uint64_t)seed >> 32);
    if ((phases & 4) && parts > 1) {
        hipLaunchKernelGGL(rl_part_kernel, dim3(parts, 2, pl.N), dim3(RL_PART_THREADS), 0, s, pl, labels, keys, s_lo, s_hi, batch_size,
                           pos_cap, counters, (int32_t*)workspace, parts);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 8) {
        if (dense_labels && hipMemsetAsync(dense_labels, 0xff, (size_t)N * pl.R, s) != hipSuccess)
            return umr_set_error(UMR_ERR_HIP, "rpn_loss: hipMemsetAsync failed");
        hipLaunchKernelGGL(rl_select_kernel, dim3(2, pl.N), dim3(RL_SELECT_THREADS), 0, s, pl, labels, matched_idxs, keys, s_lo, s_hi,
                           batch_size, pos_cap, (const int32_t*)workspace, parts, sample_index, sample_gt, counts, dense_labels, counters);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}

extern "C" int64_t umr_rpn_loss_workspace(int64_t N) {
    if (N < 1 || N > 65535) return -1;
    return N * (int64_t)sizeof(Partial);
}

extern "C" int umr_rpn_loss(const int64_t* levels, int n_levels, int64_t N, int A, int dtype, const float* cells, const float* gt_boxes,
                            const int32_t* gt_first, int64_t n_gt, const int32_t* sample_index, const int32_t* sample_gt,
                            const int32_t* counts, int batch_size, float wx, float wy, float ww, float wh, float smooth_l1_beta,
                            double scale_cls, double scale_loc, double offset, int phases, float* losses, void* workspace,
                            int64_t workspace_bytes, umr_stream_t stream) {
    RlPlan pl;
    if (int st = rl_plan(levels, 7, n_levels, N, A, offset, pl)) return st;
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "rpn_loss: logits and deltas must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(cells && gt_first && sample_index && sample_gt && counts && losses && workspace, "rpn_loss: null buffer");
    UMR_CHECK_ARG(n_gt >= 0 && n_gt < INT_MAX && (n_gt == 0 || gt_boxes), "rpn_loss: 0 <= n_gt < 2^31 - 1, and the boxes when there are any");
    UMR_CHECK_ARG(batch_size >= 1 && batch_size <= RL_MAX_BATCH, "rpn_loss: 1 <= batch_size <= 1024");
    UMR_CHECK_ARG(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f && wx <= FLT_MAX && wy <= FLT_MAX && ww <= FLT_MAX && wh <= FLT_MAX,
                  "rpn_loss: the box2box weights must be positive and finite");
    UMR_CHECK_ARG(smooth_l1_beta >= 0.f && smooth_l1_beta <= FLT_MAX, "rpn_loss: smooth_l1_beta must be >= 0 and finite");
    UMR_CHECK_ARG(scale_cls == scale_cls && scale_loc == scale_loc, "rpn_loss: a scale is NaN");
    UMR_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= (int64_t)N * (int64_t)sizeof(Partial), "rpn_loss: workspace too small or not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Partial* partials = (Partial*)workspace;
    if (phases & 1) {
        hipLaunchKernelGGL(rl_loss_kernel, dim3(pl.N), dim3(RL_THREADS), 0, s, pl, dtype, cells, gt_boxes, gt_first, (int)n_gt, sample_index,
                           sample_gt, counts, batch_size, (double)wx, (double)wy, (double)ww, (double)wh, (double)smooth_l1_beta, scale_cls,
                           scale_loc, partials);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        hipLaunchKernelGGL(rl_finish_kernel, dim3(1), dim3(RL_THREADS), 0, s, partials, pl.N, scale_cls, scale_loc, losses);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
