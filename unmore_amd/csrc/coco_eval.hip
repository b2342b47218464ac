// The two hot loops of COCO's AP / AR evaluation (pycocotools' cocoeval.py computeIoU + evaluateImg, which the reference reaches
// through COCO_evaluator/coco_evaluation.py -> COCOeval_opt): pairwise IoU of run-length masks or of boxes, and the greedy
// per-threshold matching.  An evaluation unit is one (image, category) pair: its records are D detections (already in descending
// score order) followed by G ground truths, all of one H x W.
//
// umr_mask_iou, three launches after the parse pass of rle_decode.hip (strings -> run starts):
//   mask_bits_kernel, one workgroup per record: the mask as a bit set over the format's own pixel order j = x*H + y (column-major), 64
//     pixels per word, so a run of ones is a few whole words plus two partial ones and no u8 mask exists anywhere.  A thread owns a word:
//     it finds the run that holds pixel 64*w by bisection and walks the runs that end inside the word -- no atomics, no zeroing pass.  Also
//     the record's area (popcount, integer) and the first and last non-zero word: the mask's column extent, its tight box along the
//     axis the words run along.  A malformed record (non-zero parse status) gets zero words, area 0 and an empty extent.
//   mask_iou_kernel, one workgroup per tile of MI_TD detections x MI_TG ground truths of one unit: the word range is the overlap of
//     the tile's detection extents and ground-truth extents (pairs whose columns cannot overlap cost nothing); per chunk of MI_CH words
//     the detections' words are staged in LDS, each wave takes two ground truths, a lane loads a ground-truth word once and ANDs it
//     with the MI_TD staged words: __popcll into integer accumulators, one shuffle reduction per pair at the end.
//     IoU = (double)i / (double)(a_d + a_g - i), (double)i / (double)a_d for a crowd ground truth, 0 when that denominator is 0.
// umr_box_iou: pycocotools' bbIou in its operation order, one thread per pair.
// umr_coco_match: one wave per (unit, area range, threshold); detections in order, the ground truths of the unit across the lanes.  The
//   sequential walk of evaluateImg keeps, among the eligible ground truths it visits, the LAST one of maximal IoU >= the bar (a
//   candidate replaces the held one on >=), visiting the non-ignored ones first and the ignored ones only when no non-ignored one was
//   held: two wave arg-max reductions with ties to the larger index.  "Matched" is a flag per ground truth.
//
// Contraction is off for the whole file: da + ga - w*h fused into one rounding differs from numpy / C by an ulp, and thresholds are
// compared with >=.  Everything else is integer.  No atomics, no flags between workgroups, every load and store is guarded by the
// tables' own bounds; the same input gives the same bytes on every run.
#pragma clang fp contract(off)
#include "umr_common.h"

namespace {

constexpr int CE_THREADS = 256;
constexpr int MI_TD = 8, MI_TG = 8, MI_CH = 512;    // tile: 8 detections x 8 ground truths, 512 words (4 KiB) of each per chunk: 32 KiB LDS
enum { CE_BAD_TABLE = 8 };

struct CeUnit {                                      // one unit's record range, checked
    int r0, nd, ng;
    int H, W;
    int64_t nw;                                      // words per mask
    bool ok;
};

__device__ __forceinline__ CeUnit ce_unit(const int64_t* __restrict__ unit_size, const int32_t* __restrict__ unit_start,
                                          const int32_t* __restrict__ unit_nd, int u, int K) {
    CeUnit q;
    const int r0 = unit_start[u], r1 = unit_start[u + 1], nd = unit_nd[u];
    q.ok = r0 >= 0 && r1 >= r0 && r1 <= K && nd >= 0 && nd <= r1 - r0;
    q.r0 = r0; q.nd = q.ok ? nd : 0; q.ng = q.ok ? r1 - r0 - nd : 0;
    q.H = 1; q.W = 1; q.nw = 0;
    if (unit_size) {
        const int64_t H = unit_size[u * 3 + 0], W = unit_size[u * 3 + 1];
        const bool sok = H > 0 && W > 0 && H < ((int64_t)1 << 31) && W < ((int64_t)1 << 31) && H * W < ((int64_t)1 << 31);
        if (sok) { q.H = (int)H; q.W = (int)W; q.nw = (H * W + 63) >> 6; } else { q.ok = false; q.nd = 0; q.ng = 0; }
    }
    return q;
}

// the unit of record k: the last u with unit_start[u] <= k; -1 when the table does not hold k
__device__ __forceinline__ int ce_unit_of(const int32_t* __restrict__ unit_start, int U, int k) {
    int a = 0, b = U + 1;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (unit_start[m] <= k) a = m + 1; else b = m;
    }
    return (a - 1 >= 0 && a - 1 < U) ? a - 1 : -1;
}

__global__ __launch_bounds__(CE_THREADS) void mask_bits_kernel(const int64_t* __restrict__ char_offsets, const int64_t* __restrict__ unit_size,
                                                               const int32_t* __restrict__ unit_start, const int32_t* __restrict__ unit_nd, int U,
                                                               int K, const int64_t* __restrict__ word_offsets, int64_t total_words,
                                                               int32_t* __restrict__ status, const int32_t* __restrict__ nruns,
                                                               const uint32_t* __restrict__ starts, unsigned long long* __restrict__ words,
                                                               int32_t* __restrict__ area, int32_t* __restrict__ extent) {
    __shared__ int area_w[4], lo_w[4], hi_w[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int u = ce_unit_of(unit_start, U, k);
    CeUnit q;
    q.ok = false;
    if (u >= 0) q = ce_unit(unit_size, unit_start, unit_nd, u, K);
    const int64_t wo = word_offsets[k];
    const bool slice_ok = q.ok && wo >= 0 && wo <= total_words && q.nw <= total_words - wo;
    if (!slice_ok) {                                 // workgroup-uniform: nothing of this record is ever read
        if (tid == 0) { status[k] |= CE_BAD_TABLE; area[k] = 0; extent[k * 2] = 0; extent[k * 2 + 1] = -1; }
        return;
    }
    const bool good = status[k] == 0;                // written by the parse launch
    const int n = good ? nruns[k] : 0;
    const uint32_t* s = starts + char_offsets[k] + k;
    const uint32_t HW = (uint32_t)((int64_t)q.H * q.W);
    const int nw = (int)q.nw;
    int a = 0, lo = nw, hi = -1;
    for (int w = tid; w < nw; w += CE_THREADS) {
        unsigned long long bits = 0;
        if (n > 1) {
            const uint32_t j0 = (uint32_t)w << 6, j1 = min(j0 + 64u, HW);       // HW < 2^31: no overflow
            // the last run that starts at or before j0 (starts[0] == 0)
            int x = 0, y = n;
            while (x < y) {
                const int m = (x + y) >> 1;
                if (s[m] <= j0) x = m + 1; else y = m;
            }
            for (int r = x - 1; r < n; ++r) {
                const uint32_t b = s[r], e = r + 1 < n ? s[r + 1] : HW;
                if (b >= j1) break;
                if ((r & 1) && e > b) {
                    const uint32_t p0 = max(b, j0) - j0, p1 = min(e, j1) - j0;   // bits [p0, p1), p1 > p0 whenever the run meets the word
                    if (p1 > p0) bits |= (p1 - p0 == 64 ? ~0ull : ((1ull << (p1 - p0)) - 1ull) << p0);
                }
            }
        }
        words[wo + w] = bits;
        if (bits) { a += __popcll(bits); lo = min(lo, w); hi = max(hi, w); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) { area_w[wv] = a; lo_w[wv] = lo; hi_w[wv] = hi; }
    __syncthreads();
    if (tid == 0) {
        area[k] = area_w[0] + area_w[1] + area_w[2] + area_w[3];
        extent[k * 2] = min(min(lo_w[0], lo_w[1]), min(lo_w[2], lo_w[3]));
        extent[k * 2 + 1] = max(max(hi_w[0], hi_w[1]), max(hi_w[2], hi_w[3]));
    }
}

__device__ __forceinline__ double ce_ratio(int64_t i, int64_t den) { return den > 0 ? (double)i / (double)den : 0.0; }

__global__ __launch_bounds__(CE_THREADS) void mask_iou_kernel(const int64_t* __restrict__ unit_size, const int32_t* __restrict__ unit_start,
                                                              const int32_t* __restrict__ unit_nd, int K, const int64_t* __restrict__ pair_offsets,
                                                              int64_t total_pairs, const int64_t* __restrict__ word_offsets,
                                                              const uint8_t* __restrict__ crowd, const int32_t* __restrict__ status,
                                                              const unsigned long long* __restrict__ words, const int32_t* __restrict__ area,
                                                              const int32_t* __restrict__ extent, int32_t* __restrict__ inter,
                                                              double* __restrict__ iou) {
    __shared__ unsigned long long dw[MI_TD][MI_CH];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CeUnit q = ce_unit(unit_size, unit_start, unit_nd, u, K);
    const int64_t po = pair_offsets[u];
    if (!q.ok || q.nd == 0 || q.ng == 0 || po < 0 || po > total_pairs || (int64_t)q.nd * q.ng > total_pairs - po) return;
    const int ntd = (q.nd + MI_TD - 1) / MI_TD, ntg = (q.ng + MI_TG - 1) / MI_TG;
    for (int64_t tile = blockIdx.y; tile < (int64_t)ntd * ntg; tile += gridDim.y) {          // workgroup-uniform
        const int d0 = (int)(tile / ntg) * MI_TD, g0 = (int)(tile % ntg) * MI_TG;
        const int cd = min(MI_TD, q.nd - d0), cg = min(MI_TG, q.ng - g0);
        // the tile's word range: (union of the detections' extents) meets (union of the ground truths')
        int dlo = INT_MAX, dhi = -1, glo = INT_MAX, ghi = -1;
        for (int i = 0; i < cd; ++i) {
            const int r = q.r0 + d0 + i, lo = extent[r * 2], hi = extent[r * 2 + 1];
            if (hi >= lo) { dlo = min(dlo, lo); dhi = max(dhi, hi); }
        }
        for (int j = 0; j < cg; ++j) {
            const int r = q.r0 + q.nd + g0 + j, lo = extent[r * 2], hi = extent[r * 2 + 1];
            if (hi >= lo) { glo = min(glo, lo); ghi = max(ghi, hi); }
        }
        const int wlo = max(dlo, glo), whi = min(min(dhi, ghi), (int)q.nw - 1);
        int acc[MI_TG / 4][MI_TD];
#pragma unroll
        for (int jj = 0; jj < MI_TG / 4; ++jj)
#pragma unroll
            for (int i = 0; i < MI_TD; ++i) acc[jj][i] = 0;
        if (wlo >= 0)
        for (int c0 = wlo; c0 <= whi; c0 += MI_CH) {
            for (int idx = tid; idx < MI_TD * MI_CH; idx += CE_THREADS) {
                const int i = idx / MI_CH, w = c0 + (idx % MI_CH);
                unsigned long long v = 0;
                if (i < cd) {
                    const int r = q.r0 + d0 + i;
                    if (w >= extent[r * 2] && w <= extent[r * 2 + 1]) v = words[word_offsets[r] + w];   // an extent lies inside the record's checked slice
                }
                dw[i][idx % MI_CH] = v;
            }
            __syncthreads();
#pragma unroll
            for (int jj = 0; jj < MI_TG / 4; ++jj) {
                const int j = wv + jj * 4;
                if (j < cg) {                                                   // wave-uniform
                    const int r = q.r0 + q.nd + g0 + j, lo = extent[r * 2], hi = extent[r * 2 + 1];
                    const unsigned long long* gw = words + word_offsets[r];
                    for (int x = lane; x < MI_CH; x += 64) {
                        const int w = c0 + x;
                        if (w < lo || w > hi) continue;
                        const unsigned long long g = gw[w];
                        if (!g) continue;
#pragma unroll
                        for (int i = 0; i < MI_TD; ++i) acc[jj][i] += __popcll(g & dw[i][x]);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int jj = 0; jj < MI_TG / 4; ++jj) {
            const int j = wv + jj * 4;
            int mine = 0;
#pragma unroll
            for (int i = 0; i < MI_TD; ++i) {
                const int v = wave_sum(acc[jj][i]);
                if (lane == i) mine = v;
            }
            if (j < cg && lane < cd) {
                const int rd = q.r0 + d0 + lane, rg = q.r0 + q.nd + g0 + j;
                const int64_t ad = area[rd], ag = area[rg];
                const int64_t at = po + (int64_t)(d0 + lane) * q.ng + (g0 + j);
                inter[at] = mine;
                iou[at] = ce_ratio(mine, crowd[rg] ? ad : ad + ag - mine);
            }
        }
    }
}

__global__ __launch_bounds__(CE_THREADS) void box_iou_kernel(const double* __restrict__ boxes, const int32_t* __restrict__ unit_start,
                                                             const int32_t* __restrict__ unit_nd, int K, const int64_t* __restrict__ pair_offsets,
                                                             int64_t total_pairs, const uint8_t* __restrict__ crowd, double* __restrict__ iou) {
    const int u = blockIdx.x;
    const CeUnit q = ce_unit(nullptr, unit_start, unit_nd, u, K);
    const int64_t po = pair_offsets[u], np = (int64_t)q.nd * q.ng;
    if (!q.ok || np == 0 || po < 0 || po > total_pairs || np > total_pairs - po) return;
    for (int64_t p = (int64_t)blockIdx.y * CE_THREADS + threadIdx.x; p < np; p += (int64_t)gridDim.y * CE_THREADS) {
        const int d = (int)(p / q.ng), g = (int)(p % q.ng);
        const double* D = boxes + (int64_t)(q.r0 + d) * 4;
        const double* G = boxes + (int64_t)(q.r0 + q.nd + g) * 4;
        const double da = D[2] * D[3], ga = G[2] * G[3];
        double o = 0.0;
        const double w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]);
        if (w > 0) {
            const double h = fmin(D[3] + D[1], G[3] + G[1]) - fmax(D[1], G[1]);
            if (h > 0) {
                const double i = w * h;
                const double un = crowd[q.r0 + q.nd + g] ? da : da + ga - i;
                o = i / un;
            }
        }
        iou[po + p] = o;
    }
}

__global__ __launch_bounds__(CE_THREADS) void coco_match_kernel(const double* __restrict__ iou, const int64_t* __restrict__ pair_offsets,
                                                                int64_t total_pairs, const int32_t* __restrict__ unit_nd,
                                                                const int32_t* __restrict__ unit_ng, const int64_t* __restrict__ det_offsets,
                                                                int64_t total_dets, const int64_t* __restrict__ gt_offsets, int64_t total_gts,
                                                                const double* __restrict__ dt_area, const double* __restrict__ gt_area,
                                                                const uint8_t* __restrict__ gt_crowd, const double* __restrict__ area_rng, int A,
                                                                const double* __restrict__ thr, int T, int max_det, int U,
                                                                uint8_t* __restrict__ dt_matched, int32_t* __restrict__ dt_gt,
                                                                uint8_t* __restrict__ dt_ignore, uint8_t* __restrict__ gt_ignore,
                                                                uint8_t* __restrict__ gt_matched) {
    const int lane = threadIdx.x & 63;
    const int64_t job = (int64_t)blockIdx.x * (CE_THREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
    if (job >= (int64_t)U * A * T) return;
    const int u = (int)(job / ((int64_t)A * T)), a = (int)((job / T) % A), t = (int)(job % T);
    const int D = unit_nd[u], G = unit_ng[u];
    const int64_t po = pair_offsets[u], dof = det_offsets[u], gof = gt_offsets[u];
    if (D < 0 || G < 0 || po < 0 || po > total_pairs || (int64_t)D * G > total_pairs - po || dof < 0 || dof > total_dets ||
        D > total_dets - dof || gof < 0 || gof > total_gts || G > total_gts - gof)
        return;                                                                 // a unit outside the tables is left alone
    const double lo = area_rng[a * 2], hi = area_rng[a * 2 + 1];
    const double* m = iou + po;
    const double* ga = gt_area + gof;
    const uint8_t* gc = gt_crowd + gof;
    uint8_t* gm = gt_matched + gof * A * T + ((int64_t)a * T + t) * G;           // this wave's own flags; lane g % 64 alone touches flag g
    const int64_t db = dof * A * T + ((int64_t)a * T + t) * D;
    for (int g = lane; g < G; g += 64) {
        gm[g] = 0;
        if (t == 0) gt_ignore[gof * A + (int64_t)a * G + g] = (gc[g] || ga[g] < lo || ga[g] > hi) ? 1 : 0;
    }
    const double bar = fmin(thr[t], 1 - 1e-10);
    const int ne = min(D, max_det);
    for (int d = 0; d < D; ++d) {
        if (d >= ne) {                                                          // beyond maxDet: never evaluated
            if (lane == 0) { dt_matched[db + d] = 0; dt_gt[db + d] = -1; dt_ignore[db + d] = 1; }
            continue;
        }
        double bi = -1.0;
        int bg = -1, big = 0;
        for (int pass = 0; pass < 2 && bg < 0; ++pass) {                        // bg is wave-uniform after the reduction
            bi = -1.0;
            for (int g = lane; g < G; g += 64) {
                const int c = gc[g];
                const int ig = (c || ga[g] < lo || ga[g] > hi) ? 1 : 0;
                if (ig != pass || (gm[g] && !c)) continue;
                const double v = m[(int64_t)d * G + g];
                if (v < bar) continue;
                if (v >= bi) { bi = v; bg = g; }                                // equal IoU: the later ground truth
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double oi = __shfl_xor(bi, o, 64);
                const int og = __shfl_xor(bg, o, 64);
                if (og >= 0 && (bg < 0 || oi > bi || (oi == bi && og > bg))) { bi = oi; bg = og; }
            }
            big = pass;
        }
        if (bg >= 0 && lane == (bg & 63)) gm[bg] = 1;
        if (lane == 0) {
            const double da = dt_area[dof + d];
            dt_matched[db + d] = bg >= 0;
            dt_gt[db + d] = bg;
            dt_ignore[db + d] = bg >= 0 ? big : ((da < lo || da > hi) ? 1 : 0);
        }
    }
}

int64_t ce_align8(int64_t v) { return (v + 7) & ~(int64_t)7; }
bool ce_sizes_ok(int K, int64_t total_chars, int64_t total_words) {
    return K >= 0 && total_chars >= 0 && total_words >= 0 && total_chars < ((int64_t)1 << 40) && total_words < ((int64_t)1 << 40);
}

}  // namespace

extern "C" int64_t umr_mask_iou_workspace(int K, int64_t total_chars, int64_t total_words) {
    if (!ce_sizes_ok(K, total_chars, total_words)) return -1;
    const int64_t slots = total_chars + K;
    // nruns [K] i32 | numbers [slots] i64 | run starts [slots] u32 | extents [K][2] i32 | bit words [total_words] u64
    return ce_align8((int64_t)K * 4) + slots * 8 + ce_align8(slots * 4) + (int64_t)K * 8 + total_words * 8 + 8;
}

extern "C" int umr_mask_iou(const uint8_t* chars, const int64_t* char_offsets, int K, int64_t total_chars, const int64_t* unit_size,
                            const int32_t* unit_start, const int32_t* unit_nd, const int64_t* pair_offsets, const int64_t* word_offsets,
                            const uint8_t* crowd, int U, int64_t max_pixels, int max_d, int max_g, int64_t total_pairs, int64_t total_words,
                            int32_t* inter, double* iou, int32_t* area, int32_t* status, void* workspace, int64_t workspace_bytes,
                            umr_stream_t stream) {
    UMR_CHECK_ARG(U > 0 && ce_sizes_ok(K, total_chars, total_words), "mask_iou: bad sizes");
    UMR_CHECK_ARG(max_pixels > 0 && max_pixels < ((int64_t)1 << 31), "mask_iou: H * W must be positive and below 2^31");
    UMR_CHECK_ARG(max_d >= 0 && max_g >= 0 && total_pairs >= 0, "mask_iou: negative counts");
    UMR_CHECK_ARG(unit_size && unit_start && unit_nd && pair_offsets && workspace, "mask_iou: null table or workspace");
    UMR_CHECK_ARG(K == 0 || (chars && char_offsets && word_offsets && crowd && area && status), "mask_iou: null strings, offsets, crowd, area or status");
    UMR_CHECK_ARG(total_pairs == 0 || (inter && iou), "mask_iou: null output");
    UMR_CHECK_ARG(workspace_bytes >= umr_mask_iou_workspace(K, total_chars, total_words), "mask_iou: workspace too small");
    if (K == 0) return UMR_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t slots = total_chars + K;
    char* ws = (char*)workspace;
    int32_t* nruns = (int32_t*)ws;
    long long* num = (long long*)(ws + ce_align8((int64_t)K * 4));
    uint32_t* starts = (uint32_t*)((char*)num + slots * 8);
    int32_t* extent = (int32_t*)((char*)starts + ce_align8(slots * 4));
    unsigned long long* words = (unsigned long long*)((char*)extent + (int64_t)K * 8);
    const int rc = umr_rle_parse_launch(chars, char_offsets, K, total_chars, unit_size, unit_start, U, ((int64_t)1 << 31) - 1, status, nruns, num,
                                        starts, s);
    if (rc != UMR_OK) return rc;
    hipLaunchKernelGGL(mask_bits_kernel, dim3(K), dim3(CE_THREADS), 0, s, char_offsets, unit_size, unit_start, unit_nd, U, K, word_offsets,
                       total_words, status, nruns, starts, words, area, extent);
    UMR_LAUNCH_CHECK();
    if (total_pairs > 0 && max_d > 0 && max_g > 0) {
        const int64_t tiles = (int64_t)((max_d + MI_TD - 1) / MI_TD) * ((max_g + MI_TG - 1) / MI_TG);
        hipLaunchKernelGGL(mask_iou_kernel, dim3(U, (unsigned)(tiles < 4096 ? tiles : 4096)), dim3(CE_THREADS), 0, s, unit_size, unit_start, unit_nd,
                           K, pair_offsets, total_pairs, word_offsets, crowd, status, words, area, extent, inter, iou);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}

extern "C" int umr_box_iou(const double* boxes, const int32_t* unit_start, const int32_t* unit_nd, const int64_t* pair_offsets,
                           const uint8_t* crowd, int U, int K, int64_t max_pairs, int64_t total_pairs, double* iou, umr_stream_t stream) {
    UMR_CHECK_ARG(U > 0 && K >= 0 && max_pairs >= 0 && total_pairs >= 0, "box_iou: bad sizes");
    UMR_CHECK_ARG(unit_start && unit_nd && pair_offsets, "box_iou: null table");
    UMR_CHECK_ARG(total_pairs == 0 || (boxes && crowd && iou), "box_iou: null boxes, crowd or output");
    if (total_pairs == 0 || max_pairs == 0) return UMR_OK;
    const int64_t blocks = (max_pairs + CE_THREADS - 1) / CE_THREADS;
    hipLaunchKernelGGL(box_iou_kernel, dim3(U, (unsigned)(blocks < 1024 ? blocks : 1024)), dim3(CE_THREADS), 0, (hipStream_t)stream, boxes,
                       unit_start, unit_nd, K, pair_offsets, total_pairs, crowd, iou);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_coco_match(const double* iou, const int64_t* pair_offsets, int64_t total_pairs, const int32_t* unit_nd, const int32_t* unit_ng,
                              const int64_t* det_offsets, int64_t total_dets, const int64_t* gt_offsets, int64_t total_gts, const double* dt_area,
                              const double* gt_area, const uint8_t* gt_crowd, const double* area_rng, int A, const double* thr, int T,
                              int max_det, int U, uint8_t* dt_matched, int32_t* dt_gt, uint8_t* dt_ignore, uint8_t* gt_ignore,
                              uint8_t* gt_matched, umr_stream_t stream) {
    UMR_CHECK_ARG(U > 0 && A > 0 && T > 0 && max_det >= 0 && total_pairs >= 0 && total_dets >= 0 && total_gts >= 0, "coco_match: bad sizes");
    UMR_CHECK_ARG((int64_t)U * A * T < ((int64_t)1 << 31), "coco_match: units x area ranges x thresholds must stay below 2^31");
    UMR_CHECK_ARG(pair_offsets && unit_nd && unit_ng && det_offsets && gt_offsets && area_rng && thr, "coco_match: null table");
    UMR_CHECK_ARG(total_pairs == 0 || iou, "coco_match: null IoU");
    UMR_CHECK_ARG(total_dets == 0 || (dt_area && dt_matched && dt_gt && dt_ignore), "coco_match: null detection area or output");
    UMR_CHECK_ARG(total_gts == 0 || (gt_area && gt_crowd && gt_ignore && gt_matched), "coco_match: null ground-truth area, crowd or output");
    const int64_t jobs = (int64_t)U * A * T, per = CE_THREADS / 64;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)((jobs + per - 1) / per)), dim3(CE_THREADS), 0, (hipStream_t)stream, iou, pair_offsets,
                       total_pairs, unit_nd, unit_ng, det_offsets, total_dets, gt_offsets, total_gts, dt_area, gt_area, gt_crowd, area_rng, A, thr,
                       T, max_det, U, dt_matched, dt_gt, dt_ignore, gt_ignore, gt_matched);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
