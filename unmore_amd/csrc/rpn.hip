// The proposal step of the stage-3 detector's RPN (cad/modeling/meta_arch/rcnn.py:165, 213, 333: self.proposal_generator(...), which
// is Detectron2's RPN.predict_proposals -> _decode_proposals + find_top_rpn_proposals): the head's raw objectness logits [N,A,H,W] and
// anchor deltas [N,4A,H,W] of every pyramid level, read in place -> per image the proposals that survive the per-level top-k, the
// decode, the clip, the drop of non-finite and empty boxes, the per-level NMS and the merge, with their logits.
//
// Five launches for the whole batch, nothing read back, no float atomics (integer LDS atomics build histograms and counts: integer sums
// have no order), the same input gives the same bytes.  The level descriptors travel in the kernels' arguments.
//   rpn_part_kernel    one workgroup of 256 threads per (part, level, image), only for levels of more than RPN_SELECT_SHARE scores: the
//                      top min(K, share) of the part's scores by select_in_order.h's radix select over order-preserving keys, compacted
//                      IN f ORDER (key and flat index f) into the workspace; the parts of a level lie one after the other, so their
//                      concatenation is again in f order.
//   rpn_rank_kernel    one workgroup of 1024 threads per (level, image): the same select over the level's scores (one part) or over its
//                      parts' survivors, K of them in f order into LDS; every one counts its rank #{j : key_j > key_i or (key_j == key_i
//                      and j < i)} (a permutation), decodes its anchor and writes the clipped box, the logit, f and a flag to rank's slot.
//   rpn_mask_kernel    one wave per 64 x 64 tile of a level's upper triangle: the suppression matrix of nms_bitmask.h, no predicate.
//   rpn_scan_kernel    one wave per (level, image): nms_bitmask.h's greedy scan from the level's valid set, one word per lane
//                      (K <= 4096), no limit.  The kept boxes and logits are written compacted, in rank order.
//   rpn_merge_kernel   a thread per kept candidate: its place in the image's order = its place in its level + the number of kept
//                      candidates of every lower level with logit >= its own + of every higher level with logit > its own (bisection in
//                      the levels' sorted lists); the first post_nms_topk are written.
// Order of the scores: key(v) = 0xffffffff for a NaN; else with u = bits(v == 0 ? +0 : v): u < 0 ? ~u : u | 0x80000000.  Larger key =
// larger value, a NaN above +inf, -0.0 == +0.0 (torch.topk's order); equal keys in ascending f = (y * W + x) * A + a.
// Arithmetic, float32, no contraction, every operation rounded on its own (det_box.h: grid_anchor, box_apply_deltas, box_clip; the
// suppression's IoU and its strict `>`: nms_bitmask.h):
//   anchor      sx = float(x * stride) + off, sy = float(y * stride) + off  (off = offset * stride, exact);  (sx + c0, sy + c1, sx + c2, sy + c3)
//               for the level's cell anchor c of index a
//   apply       w = x2 - x1; cx = x1 + .5 w; dx = dx / wx; dw = min(dw / ww, log(1000 / 16)); pcx = dx * w + cx; pw = expf(dw) * w;
//               x1' = pcx - .5 pw; x2' = pcx + .5 pw   (Box2BoxTransform.apply_deltas; bfloat16 deltas widened)
//   non-finite  a decoded coordinate or the logit is NaN or +-inf: dropped and counted (flag 1)
//   clip        x < 0 ? 0 : (x > width ? width : x)
//   empty       not (x2 - x1 > min_box_size and y2 - y1 > min_box_size) after the clip: dropped and counted (flag 2)
#pragma clang fp contract(off)
#include "umr_common.h"
#include "det_box.h"
#include "nms_bitmask.h"
#include "select_in_order.h"
#include <algorithm>
#include <float.h>
#include <limits.h>

namespace {

constexpr int RPN_MAX_LEVELS = 8;
constexpr int RPN_MAX_A = 16;                         // anchors per position the host accepts (rpn.py: MAX_ANCHORS)
constexpr int RPN_MAX_K = 4096;                       // pre_nms_topk: 64 words of removed set = one per lane of the scanning wave
constexpr int RPN_SELECT_SHARE = 16384;               // scores per workgroup of rpn_part_kernel
constexpr int RPN_PART_THREADS = 256;
constexpr int RPN_RANK_THREADS = 1024;

static_assert(RPN_MAX_A == GRID_MAX_A, "the cells table [L, GRID_MAX_A, 4] has a row for every anchor the host accepts");

struct RpnLevel {
    const void* logits;               // [N,A,H,W]
    const void* deltas;               // [N,4A,H,W]
    int H, W, stride, K;              // K = min(H * W * A, pre_nms_topk)
    int n;                            // H * W * A
    int parts;                        // ceil(n / RPN_SELECT_SHARE)
    int cand_first;                   // the sum of K over the levels before
    int part_len;                     // parts == 1: 0; else (parts - 1) * K + min(K, n - (parts - 1) * share)
    long long part_first;             // per image: the sum of part_len over the levels before
    long long mat_first;              // per image: the sum of K * ceil(K / 64) over the levels before
    float off;                        // offset * stride
    int pad;
};

struct RpnPlan {
    RpnLevel lv[RPN_MAX_LEVELS];
    int L, N, A, dtype, cand_total, max_K, max_parts, cap;
    long long part_total, mat_total;  // per image
};

struct RpnWork {
    unsigned* pkey; int32_t* pidx;                    // [N, part_total]
    unsigned long long* mat;                          // [N, mat_total]
    unsigned long long* valid;                        // [N, L, 64]
    f32x4* kbox; float* kscore; int32_t* nkept;       // [N, cand_total], [N, L]
};

__device__ __forceinline__ unsigned rpn_key(float v) {
    if (v != v) return 0xffffffffu;
    if (v == 0.f) return 0x80000000u;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float rpn_load(const void* p, int dtype, int64_t at) {
    return dtype == UMR_BF16 ? (float)((const bf16_t*)p)[at] : ((const float*)p)[at];
}

// the sequence a select reads: the scores f0 ... of one image's level straight from the head's output, or a list of (key, f)
struct RpnSrc {
    const void* logits; int dtype, A, HW; int64_t img; int f0;
    const unsigned* pkey; const int32_t* pidx;
    __device__ __forceinline__ unsigned key(int i) const {
        if (pkey) return pkey[i];
        const int f = f0 + i, pix = f / A, a = f - pix * A;
        return rpn_key(rpn_load(logits, dtype, img + (int64_t)a * HW + pix));
    }
    __device__ __forceinline__ int idx(int i) const { return pkey ? pidx[i] : f0 + i; }
};

// what a select of the scores keeps of its j-th entry: the key and the flat index f.  rpn_key never returns 0 (a NaN maps to
// 0xffffffff, +-0 to 0x80000000, a negative to ~u >= 0x007fffff), so select_in_order's "key 0 takes no part" cannot drop a score.
struct RpnKeep {
    const RpnSrc& src; unsigned* key; int32_t* idx;
    __device__ __forceinline__ void operator()(int j, int i, unsigned k) const { key[j] = k; idx[j] = src.idx(i); }
};

__global__ __launch_bounds__(RPN_PART_THREADS) void rpn_part_kernel(RpnPlan pl, RpnWork ws) {
    __shared__ int hist[256];
    __shared__ int wtot[32];
    const int part = blockIdx.x, l = blockIdx.y, n = blockIdx.z;
    const RpnLevel lv = pl.lv[l];
    if (lv.parts <= 1 || part >= lv.parts) return;
    const int f0 = part * RPN_SELECT_SHARE, cnt = min(RPN_SELECT_SHARE, lv.n - f0), k = min(lv.K, cnt);
    const RpnSrc src{lv.logits, pl.dtype, pl.A, lv.H * lv.W, (int64_t)n * pl.A * lv.H * lv.W, f0, nullptr, nullptr};
    const long long at = (long long)n * pl.part_total + lv.part_first + (long long)part * lv.K;
    (void)select_in_order(src, cnt, k, hist, wtot, RpnKeep{src, ws.pkey + at, ws.pidx + at});
}

__global__ __launch_bounds__(RPN_RANK_THREADS) void rpn_rank_kernel(RpnPlan pl, RpnWork ws, const float* __restrict__ cells,
                                                                   const float* __restrict__ image_sizes, f32x4 bw, float min_box_size,
                                                                   f32x4* __restrict__ cbox, float* __restrict__ cscore,
                                                                   int32_t* __restrict__ cidx, uint8_t* __restrict__ cflag,
                                                                   f32x4* __restrict__ craw, int32_t* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) unsigned s_key[RPN_MAX_K];
    __shared__ int32_t s_idx[RPN_MAX_K];
    __shared__ unsigned long long s_valid[64];
    __shared__ int hist[256];
    __shared__ int wtot[32];
    __shared__ int s_bad[2];
    const int l = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const RpnLevel lv = pl.lv[l];
    const int K = lv.K, HW = lv.H * lv.W;
    const int64_t img = (int64_t)n * pl.A * HW;
    if (tid < 64) s_valid[tid] = 0ull;
    if (tid < 2) s_bad[tid] = 0;
    if (lv.parts <= 1) {
        const RpnSrc src{lv.logits, pl.dtype, pl.A, HW, img, 0, nullptr, nullptr};
        (void)select_in_order(src, lv.n, K, hist, wtot, RpnKeep{src, s_key, s_idx});
    } else {
        const long long at = (long long)n * pl.part_total + lv.part_first;
        const RpnSrc src{nullptr, 0, 1, 1, 0, 0, ws.pkey + at, ws.pidx + at};
        (void)select_in_order(src, lv.part_len, K, hist, wtot, RpnKeep{src, s_key, s_idx});
    }
    const float height = image_sizes[n * 2], width = image_sizes[n * 2 + 1];
    const int64_t cb = (int64_t)n * pl.cand_total + lv.cand_first;
    const int K4 = K & ~3;
    for (int i = tid; i < K; i += RPN_RANK_THREADS) {
        const unsigned ki = s_key[i];
        int rank = 0;                                               // det_post.hip's dp_candidates_kernel counts the same on scores
        for (int j = 0; j < K4; j += 4) {
            const u32x4 v = *(const u32x4*)(s_key + j);
            rank += (v[0] > ki || (v[0] == ki && j < i)) + (v[1] > ki || (v[1] == ki && j + 1 < i)) +
                    (v[2] > ki || (v[2] == ki && j + 2 < i)) + (v[3] > ki || (v[3] == ki && j + 3 < i));
        }
        for (int j = K4; j < K; ++j) {
            const unsigned kj = s_key[j];
            rank += (kj > ki || (kj == ki && j < i));
        }
        int f = s_idx[i];
        if (f < 0 || f >= lv.n) f = 0;                              // never: the indices are this call's own
        const int pix = f / pl.A, a = f - pix * pl.A, y = pix / lv.W, x = pix - y * lv.W;
        const float wt[4] = {bw[0], bw[1], bw[2], bw[3]};           // here, not before the loop: there it cost the rank count its schedule
        float anchor[4], r[4];
        grid_anchor(cells + (l * GRID_MAX_A + a) * 4, x, y, lv.stride, lv.off, anchor);
        const int64_t dat = (int64_t)n * 4 * pl.A * HW + (int64_t)(a * 4) * HW + pix;
        const float d[4] = {rpn_load(lv.deltas, pl.dtype, dat), rpn_load(lv.deltas, pl.dtype, dat + HW),
                            rpn_load(lv.deltas, pl.dtype, dat + 2 * (int64_t)HW), rpn_load(lv.deltas, pl.dtype, dat + 3 * (int64_t)HW)};
        const float score = rpn_load(lv.logits, pl.dtype, img + (int64_t)a * HW + pix);
        box_apply_deltas(d, anchor, wt, r);
        const f32x4 raw = {r[0], r[1], r[2], r[3]};
        const bool fin = box_finite(raw[0]) && box_finite(raw[1]) && box_finite(raw[2]) && box_finite(raw[3]) && box_finite(score);
        const f32x4 box = {box_clip(raw[0], width), box_clip(raw[1], height), box_clip(raw[2], width), box_clip(raw[3], height)};
        const bool full = (box[2] - box[0] > min_box_size) && (box[3] - box[1] > min_box_size);
        const int flag = !fin ? 1 : (!full ? 2 : 0);
        if (rank < K) {                                             // a permutation of [0, K): always
            cbox[cb + rank] = box;
            cscore[cb + rank] = score;
            cidx[cb + rank] = f;
            cflag[cb + rank] = (uint8_t)flag;
            if (craw) craw[cb + rank] = raw;
            if (flag == 0) atomicOr(&s_valid[rank >> 6], 1ull << (rank & 63));
            else atomicAdd(&s_bad[flag - 1], 1);
        }
    }
    __syncthreads();
    if (tid < 64) ws.valid[((int64_t)n * pl.L + l) * 64 + tid] = s_valid[tid];
    if (tid < 3) stats[((int64_t)n * pl.L + l) * 5 + tid] = tid == 0 ? K : s_bad[tid - 1];
}

__global__ __launch_bounds__(64) void rpn_mask_kernel(RpnPlan pl, RpnWork ws, float nms_thresh, const f32x4* __restrict__ cbox) {
    __shared__ f32x4 tile[64];
    const int l = blockIdx.z % pl.L, n = blockIdx.z / pl.L, rb = blockIdx.y, cbk = blockIdx.x, t = threadIdx.x;
    const RpnLevel lv = pl.lv[l];
    const int K = lv.K, words = (K + 63) >> 6;
    if (cbk < rb || rb * 64 >= K || cbk * 64 >= K) return;          // the upper triangle of the ranks that exist
    const int64_t cb = (int64_t)n * pl.cand_total + lv.cand_first;
    const int j0 = cbk * 64, nj = min(64, K - j0);
    if (t < nj) tile[t] = cbox[cb + j0 + t];
    __syncthreads();
    const int i = rb * 64 + t;
    if (i >= K) return;
    const unsigned long long bits = nms_tile_word(cbox[cb + i], i, tile, j0, nj, nms_thresh, NmsAlways{});
    ws.mat[(long long)n * pl.mat_total + lv.mat_first + (long long)i * words + cbk] = bits;
}

__global__ __launch_bounds__(64) void rpn_scan_kernel(RpnPlan pl, RpnWork ws, const f32x4* __restrict__ cbox,
                                                      const float* __restrict__ cscore, int32_t* __restrict__ stats) {
    __shared__ int kept_rank[RPN_MAX_K];
    const int l = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    const RpnLevel lv = pl.lv[l];
    const int K = lv.K, words = (K + 63) >> 6;
    const unsigned long long* mat = ws.mat + (long long)n * pl.mat_total + lv.mat_first;
    unsigned long long val[1] = {ws.valid[((int64_t)n * pl.L + l) * 64 + lane] & nms_all_valid(lane, K)};
    const int kept = nms_greedy_scan<1>(mat, words, words, K, val, INT_MAX, kept_rank);
    __syncthreads();
    const int n_valid = wave_sum(__popcll(val[0]));
    const int64_t cb = (int64_t)n * pl.cand_total + lv.cand_first;
    for (int j = lane; j < kept; j += 64) {
        const int r = kept_rank[j];
        ws.kbox[cb + j] = cbox[cb + r];
        ws.kscore[cb + j] = cscore[cb + r];
    }
    if (lane == 0) {
        ws.nkept[n * pl.L + l] = kept;
        stats[((int64_t)n * pl.L + l) * 5 + 3] = n_valid - kept;
        stats[((int64_t)n * pl.L + l) * 5 + 4] = kept;
    }
}

// #{j : s[j] > v} (strict) or #{j : s[j] >= v} of a list in descending order
__device__ __forceinline__ int rpn_count_before(const float* __restrict__ s, int len, float v, bool strict) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float m = s[mid];
        if (strict ? m > v : m >= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void rpn_merge_kernel(RpnPlan pl, RpnWork ws, float* __restrict__ out_boxes, float* __restrict__ out_logits,
                                                        int32_t* __restrict__ counts) {
    const int n = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s == 0) {
        int total = 0;
        for (int l = 0; l < pl.L; ++l) total += min(max(ws.nkept[n * pl.L + l], 0), pl.lv[l].K);
        counts[n] = min(total, pl.cap);
    }
    if (s >= pl.cand_total) return;
    int l = 0;
    while (l + 1 < pl.L && s >= pl.lv[l + 1].cand_first) ++l;
    const int j = s - pl.lv[l].cand_first;
    if (j >= min(ws.nkept[n * pl.L + l], pl.lv[l].K)) return;
    const int64_t ib = (int64_t)n * pl.cand_total;
    const float v = ws.kscore[ib + s];
    int pos = j;
    for (int o = 0; o < pl.L; ++o) {
        if (o == l) continue;
        const int len = min(max(ws.nkept[n * pl.L + o], 0), pl.lv[o].K);
        pos += rpn_count_before(ws.kscore + ib + pl.lv[o].cand_first, len, v, o > l);
    }
    if (pos < pl.cap) {
        *(f32x4*)(out_boxes + ((int64_t)n * pl.cap + pos) * 4) = ws.kbox[ib + s];
        out_logits[(int64_t)n * pl.cap + pos] = v;
    }
}

// the plan of a call from the host array of levels (5 int64 each: logits, deltas, H, W, stride); UMR_OK or the error set
int rpn_plan(const int64_t* levels, int n_levels, int64_t N, int A, int dtype, int pre_nms_topk, int post_nms_topk, double offset, bool pointers,
             RpnPlan& pl) {
    UMR_CHECK_ARG(levels && n_levels >= 1 && n_levels <= RPN_MAX_LEVELS, "rpn: between 1 and 8 levels");
    UMR_CHECK_ARG(N >= 1 && N <= 65535, "rpn: between 1 and 65535 images");
    UMR_CHECK_ARG(A >= 1 && A <= RPN_MAX_A, "rpn: between 1 and 16 anchors per position");
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "rpn: logits and deltas must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(pre_nms_topk >= 1 && pre_nms_topk <= RPN_MAX_K, "rpn: pre_nms_topk must lie in [1, 4096]");
    UMR_CHECK_ARG(post_nms_topk >= 1, "rpn: post_nms_topk must be positive");
    UMR_CHECK_ARG(offset >= 0.0 && offset < 1.0, "rpn: offset must lie in [0, 1)");
    pl = RpnPlan{};
    pl.L = n_levels; pl.N = (int)N; pl.A = A; pl.dtype = dtype;
    for (int l = 0; l < n_levels; ++l) {
        const int64_t* e = levels + 5 * l;
        RpnLevel& lv = pl.lv[l];
        UMR_CHECK_ARG(!pointers || (e[0] && e[1]), "rpn: a level without logits or deltas");
        UMR_CHECK_ARG(e[2] >= 1 && e[3] >= 1 && e[2] <= INT_MAX && e[3] <= INT_MAX && e[2] * e[3] <= INT_MAX / A - 1,
                      "rpn: a level needs 0 < H * W * A < 2^31");
        UMR_CHECK_ARG(e[4] >= 1 && e[4] <= (1 << 24) && e[2] * e[4] <= (1 << 24) && e[3] * e[4] <= (1 << 24),
                      "rpn: a stride must be positive with H * stride and W * stride at most 2^24");
        lv.logits = (const void*)(uintptr_t)e[0];
        lv.deltas = (const void*)(uintptr_t)e[1];
        lv.H = (int)e[2]; lv.W = (int)e[3]; lv.stride = (int)e[4];
        lv.n = lv.H * lv.W * A;
        lv.K = std::min(lv.n, pre_nms_topk);
        lv.parts = (lv.n + RPN_SELECT_SHARE - 1) / RPN_SELECT_SHARE;
        lv.cand_first = pl.cand_total;
        lv.part_first = pl.part_total;
        lv.mat_first = pl.mat_total;
        lv.part_len = lv.parts > 1 ? (lv.parts - 1) * lv.K + std::min(lv.K, lv.n - (lv.parts - 1) * RPN_SELECT_SHARE) : 0;
        lv.off = (float)(offset * (double)lv.stride);                 // exact: the caller checks that the product is a float32 value
        pl.cand_total += lv.K;
        pl.part_total += lv.part_len;
        pl.mat_total += (long long)lv.K * ((lv.K + 63) / 64);
        pl.max_K = std::max(pl.max_K, lv.K);
        pl.max_parts = std::max(pl.max_parts, lv.parts > 1 ? lv.parts : 0);
    }
    pl.cap = std::min(post_nms_topk, pl.cand_total);
    return UMR_OK;
}

inline int64_t rpn_up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

int64_t rpn_workspace_bytes(const RpnPlan& pl) {
    const int64_t N = pl.N, c = N * pl.cand_total, p = std::max<int64_t>(N * pl.part_total, 1);
    return rpn_up16(p * 4) * 2 + rpn_up16(N * pl.mat_total * 8) + N * pl.L * 64 * 8 + c * 16 + rpn_up16(c * 4) + rpn_up16(N * pl.L * 4);
}

}  // namespace

extern "C" int64_t umr_rpn_workspace(const int64_t* levels, int n_levels, int64_t N, int A, int pre_nms_topk) {
    RpnPlan pl;
    if (rpn_plan(levels, n_levels, N, A, UMR_F32, pre_nms_topk, 1, 0.0, false, pl) != UMR_OK) return -1;
    return rpn_workspace_bytes(pl);
}

extern "C" int umr_rpn_proposals(const int64_t* levels, int n_levels, int64_t N, int A, int dtype, const float* cells,
                                 const float* image_sizes, int pre_nms_topk, int post_nms_topk, float nms_thresh, float min_box_size,
                                 float wx, float wy, float ww, float wh, double offset, int phases, float* cand_boxes, float* cand_scores,
                                 int32_t* cand_idx, uint8_t* cand_flags, float* cand_raw, float* out_boxes, float* out_logits,
                                 int32_t* counts, int32_t* stats, void* workspace, int64_t workspace_bytes, umr_stream_t stream) {
    RpnPlan pl;
    if (int st = rpn_plan(levels, n_levels, N, A, dtype, pre_nms_topk, post_nms_topk, offset, true, pl)) return st;
    UMR_CHECK_ARG(cells && image_sizes, "rpn: the cell anchors [L,16,4] and the image sizes [N,2] on the device");
    UMR_CHECK_ARG(nms_thresh == nms_thresh && min_box_size == min_box_size, "rpn: a threshold is NaN");
    UMR_CHECK_ARG(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f && wx <= FLT_MAX && wy <= FLT_MAX && ww <= FLT_MAX && wh <= FLT_MAX,
                  "rpn: the box2box weights must be positive and finite");
    UMR_CHECK_ARG(cand_boxes && cand_scores && cand_idx && cand_flags && out_boxes && out_logits && counts && stats && workspace,
                  "rpn: null buffer");
    UMR_CHECK_ARG((((uintptr_t)cand_boxes | (uintptr_t)cand_raw | (uintptr_t)out_boxes | (uintptr_t)workspace) & 15) == 0,
                  "rpn: a box buffer or the workspace is not 16-byte aligned");
    UMR_CHECK_ARG((int64_t)N * pl.cand_total <= INT_MAX, "rpn: 2^31 candidates or more in the batch");
    UMR_CHECK_ARG(workspace_bytes >= rpn_workspace_bytes(pl), "rpn: workspace too small");
    const int64_t c = (int64_t)N * pl.cand_total, p = std::max<int64_t>((int64_t)N * pl.part_total, 1);
    unsigned char* base = (unsigned char*)workspace;
    RpnWork ws;
    ws.pkey = (unsigned*)base;                 base += rpn_up16(p * 4);
    ws.pidx = (int32_t*)base;                  base += rpn_up16(p * 4);
    ws.mat = (unsigned long long*)base;        base += rpn_up16((int64_t)N * pl.mat_total * 8);
    ws.valid = (unsigned long long*)base;      base += (int64_t)N * pl.L * 64 * 8;
    ws.kbox = (f32x4*)base;                    base += c * 16;
    ws.kscore = (float*)base;                  base += rpn_up16(c * 4);
    ws.nkept = (int32_t*)base;
    hipStream_t s = (hipStream_t)stream;
    const f32x4 bw = {wx, wy, ww, wh};
    if ((phases & 1) && pl.max_parts > 0) {
        hipLaunchKernelGGL(rpn_part_kernel, dim3(pl.max_parts, pl.L, pl.N), dim3(RPN_PART_THREADS), 0, s, pl, ws);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        hipLaunchKernelGGL(rpn_rank_kernel, dim3(pl.L, pl.N), dim3(RPN_RANK_THREADS), 0, s, pl, ws, cells, image_sizes, bw, min_box_size,
                           (f32x4*)cand_boxes, cand_scores, cand_idx, cand_flags, (f32x4*)cand_raw, stats);
        UMR_LAUNCH_CHECK();
    }
    const int tiles = (pl.max_K + 63) / 64;
    if (phases & 4) {
        UMR_CHECK_ARG((int64_t)pl.L * pl.N <= 65535, "rpn: levels x images above 65535");
        hipLaunchKernelGGL(rpn_mask_kernel, dim3(tiles, tiles, pl.L * pl.N), dim3(64), 0, s, pl, ws, nms_thresh, (const f32x4*)cand_boxes);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 8) {
        hipLaunchKernelGGL(rpn_scan_kernel, dim3(pl.L, pl.N), dim3(64), 0, s, pl, ws, (const f32x4*)cand_boxes, cand_scores, stats);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 16) {
        hipLaunchKernelGGL(rpn_merge_kernel, dim3((pl.cand_total + 255) / 256, pl.N), dim3(256), 0, s, pl, ws, out_boxes, out_logits, counts);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
