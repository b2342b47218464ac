// The box branch of the stage-3 detector's cascade ROI heads (cad/modeling/roi_heads/custom_cascade_rcnn.py:166-357 and
// fast_rcnn.py:94-121, 329-390, 462-514, 574-598; cad/structures/boxes.py; cad/modeling/box_regression.py): matching and labelling of a
// stage's proposals, the decode / clip / drop-empty of its predictions into the next stage's proposals, the drop-loss weights, and the
// two losses of FastRCNNOutputLayers with their gradients and logged counts.
//
// All kernels walk the same table (include/umr.h, umr_bl_image): one entry per image, its proposals cut into chunks of 256 rows, one
// workgroup of 256 threads per chunk, a thread per proposal; a workgroup finds its image by bisection on chunk_first (entries without
// proposals share a chunk_first with the entry after them and are never found).  No atomics on floats: per-workgroup partials go into a
// workspace and a finishing launch of one workgroup adds them in index order, so the same input gives the same bytes.  (The matcher's
// per-image counts are int32 and use one integer atomic per workgroup: integer sums have no order.)
//
//   bl_match_kernel    stages the image's ground truths in LDS in tiles of BL_GT_TILE boxes with their areas; each thread walks the tile
//                      for its proposal in index order and keeps the first maximum (`>`), as torch's CPU max(dim=0) does.
//   bl_decode_kernel   apply_deltas + clip + nonempty per row into a temporary, and the chunk's number of kept rows.
//   bl_compact_kernel  per chunk: the kept rows of all chunks before it (summed in index order), a wave-ballot prefix scan inside the
//                      chunk, then the scatter; order is preserved.  Workgroup 0 also writes the per-image counts.
//   bl_loss_kernel     per chunk: the image's drop-loss ground-truth set (distinct rows among its first 100 matched boxes, at most
//                      100 x 100 row comparisons, in LDS), the row's drop weight, its cross-entropy term, its box-regression term, both
//                      gradients and the seven counts; one partial per workgroup.
//   bl_finish_kernel   sums the partials: the two losses as float32, the counts as int64.
//
// Arithmetic, float32, no contraction, every operation rounded on its own (det_box.h, shared with the other detector kernels):
//   iou(a, b)   = inter > 0 ? inter / ((area_a + area_b) - inter) : 0,  inter = max(min(a.x2, b.x2) - max(a.x1, b.x1), 0) * (same in y),
//                 area = (x2 - x1) * (y2 - y1); the division is correctly rounded, so the value equals a float32 NumPy restatement bit for bit.
//   apply       w = x2 - x1; cx = x1 + .5 w; dx = dx / wx; dw = min(dw / ww, log(1000 / 16)); pcx = dx * w + cx; pw = expf(dw) * w;
//               x1' = pcx - .5 pw; x2' = pcx + .5 pw   (Detectron2's Box2BoxTransform.apply_deltas)
//   get         dx = wx * (tcx - scx) / sw; dw = ww * logf(tw / sw)   (Box2BoxTransform.get_deltas)
#pragma clang fp contract(off)
#include "umr_common.h"
#include "det_box.h"
#include <algorithm>
#include <float.h>

namespace {

constexpr int BL_THREADS = 256;
constexpr int BL_GT_TILE = 256;                       // ground truths staged in LDS at a time (== BL_THREADS: one load per thread)
constexpr int BL_UNIQUE_ROWS = 100;                   // the reference's gt_boxes.tensor[:100]

struct BlW { float v[4]; };                           // the Box2BoxTransform weights (wx, wy, ww, wh)

static_assert(sizeof(umr_bl_image) == 56 && offsetof(umr_bl_image, width) == 52, "umr_bl_image is mirrored by _lib.BlImage");

using Partial = SumPartial<2, 7>;                     // one per workgroup, 48 bytes: the classification and the box sum; rows, fg, pred == gt,
                                                      // fg & pred == gt, fg & pred == bg, dropped, bad

__device__ __forceinline__ int bl_find(const umr_bl_image* __restrict__ images, int n_images, int chunk) {
    int lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (images[mid].chunk_first <= chunk) lo = mid; else hi = mid;
    }
    return lo;
}

// what the kernels trust of a table entry before they index with it
__device__ __forceinline__ bool bl_entry_ok(const umr_bl_image& im, int chunk, int R) {
    return im.R >= 0 && im.first >= 0 && im.first <= R - im.R && im.G >= 0 && chunk >= im.chunk_first &&
           (int64_t)(chunk - im.chunk_first) * BL_THREADS < im.R && im.boxes;
}

// the sum of v over the workgroup, in every thread; red: 4 ints of LDS
__device__ __forceinline__ int bl_block_sum(int v, int* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---------------------------------------------------------------------------------------------------------------- match and label
__global__ __launch_bounds__(BL_THREADS) void bl_match_kernel(const umr_bl_image* __restrict__ images, int n_images, int R, float threshold,
                                                              long long num_classes, int64_t* __restrict__ matched_idxs,
                                                              float* __restrict__ matched_vals, int64_t* __restrict__ out_classes,
                                                              float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                              int32_t* __restrict__ counts) {
    __shared__ float gt[BL_GT_TILE][5];                                   // x1 y1 x2 y2 area
    __shared__ int red[4];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const int k = bl_find(images, n_images, chunk);
    const umr_bl_image im = images[k];
    if (!bl_entry_ok(im, chunk, R) || (im.G > 0 && !(im.gt_boxes && im.gt_classes && im.gt_scores))) return;   // workgroup-uniform
    const int j = (chunk - im.chunk_first) * BL_THREADS + tid;
    const bool live = j < im.R;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float* b = im.boxes + (int64_t)j * 4;
        p[0] = b[0]; p[1] = b[1]; p[2] = b[2]; p[3] = b[3];
    }
    const bool bad = live && !(box_finite(p[0]) && box_finite(p[1]) && box_finite(p[2]) && box_finite(p[3]));
    const float p_area = box_area(p[0], p[1], p[2], p[3]);
    float best = -1.f;
    int best_g = 0;
    for (int g0 = 0; g0 < im.G; g0 += BL_GT_TILE) {
        const int n = min(BL_GT_TILE, im.G - g0);
        __syncthreads();
        if (tid < n) {
            const float* b = im.gt_boxes + (int64_t)(g0 + tid) * 4;
            gt[tid][0] = b[0]; gt[tid][1] = b[1]; gt[tid][2] = b[2]; gt[tid][3] = b[3];
            gt[tid][4] = box_area(b[0], b[1], b[2], b[3]);
        }
        __syncthreads();
        if (live && !bad) {
            for (int g = 0; g < n; ++g) {
                const float v = box_iou_match(gt[g][0], gt[g][1], gt[g][2], gt[g][3], gt[g][4], p[0], p[1], p[2], p[3], p_area);
                // strict: the lowest index that attains the maximum.  A NaN (a ground truth that is not finite) never wins, where
                // torch's max would hand it on: include/umr.h names the departure
                if (v > best) { best = v; best_g = g0 + g; }
            }
        }
    }
    const bool matched = live && !bad && im.G > 0 && best >= 0.f;
    const bool fg = matched && best >= threshold;
    if (live) {
        const int64_t r = (int64_t)im.first + j;
        matched_idxs[r] = best_g;
        matched_vals[r] = matched ? best : 0.f;
        float* ob = out_boxes + r * 4;
        if (im.G > 0) {
            const float* b = im.gt_boxes + (int64_t)best_g * 4;
            ob[0] = b[0]; ob[1] = b[1]; ob[2] = b[2]; ob[3] = b[3];
            out_scores[r] = im.gt_scores[best_g];
            out_classes[r] = fg ? im.gt_classes[best_g] : num_classes;
        } else {
            ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
            out_scores[r] = 0.f;
            out_classes[r] = num_classes;
        }
    }
    const int n_fg = bl_block_sum(fg ? 1 : 0, red);
    const int n_bad = bl_block_sum(bad ? 1 : 0, red);
    if (tid == 0) {
        const int rows = min(BL_THREADS, im.R - (chunk - im.chunk_first) * BL_THREADS);
        if (n_fg) atomicAdd(counts + k, n_fg);
        if (rows - n_fg) atomicAdd(counts + n_images + k, rows - n_fg);
        if (n_bad) atomicAdd(counts + 2 * n_images + k, n_bad);
    }
}

// ---------------------------------------------------------------------------------------------------------------- decode and compact
template <typename T>
__global__ __launch_bounds__(BL_THREADS) void bl_decode_kernel(const umr_bl_image* __restrict__ images, int n_images, int R,
                                                               const T* __restrict__ deltas, BlW bw, int training,
                                                               float* __restrict__ tmp, uint8_t* __restrict__ keep,
                                                               int32_t* __restrict__ chunk_counts) {
    __shared__ int red[4];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const umr_bl_image im = images[bl_find(images, n_images, chunk)];
    if (!bl_entry_ok(im, chunk, R)) {
        if (tid == 0) chunk_counts[chunk] = 0;
        return;
    }
    const int j = (chunk - im.chunk_first) * BL_THREADS + tid;
    int kept = 0;
    if (j < im.R) {
        const int64_t r = (int64_t)im.first + j;
        const float* b = im.boxes + (int64_t)j * 4;
        const float box[4] = {b[0], b[1], b[2], b[3]};
        const float d[4] = {to_f32<T>(deltas[r * 4]), to_f32<T>(deltas[r * 4 + 1]), to_f32<T>(deltas[r * 4 + 2]), to_f32<T>(deltas[r * 4 + 3])};
        float o[4];
        box_apply_deltas(d, box, bw.v, o);
        o[0] = box_clip(o[0], im.width);
        o[1] = box_clip(o[1], im.height);
        o[2] = box_clip(o[2], im.width);
        o[3] = box_clip(o[3], im.height);
        kept = !training || ((o[2] - o[0]) > 0.f && (o[3] - o[1]) > 0.f);
        tmp[r * 4] = o[0]; tmp[r * 4 + 1] = o[1]; tmp[r * 4 + 2] = o[2]; tmp[r * 4 + 3] = o[3];
        keep[r] = (uint8_t)kept;
    }
    const int total = bl_block_sum(kept, red);
    if (tid == 0) chunk_counts[chunk] = total;
}

__global__ __launch_bounds__(BL_THREADS) void bl_compact_kernel(const umr_bl_image* __restrict__ images, int n_images, int R, int n_chunks,
                                                                const float* __restrict__ tmp, const uint8_t* __restrict__ keep,
                                                                const int32_t* __restrict__ chunk_counts, float* __restrict__ out,
                                                                int32_t* __restrict__ counts) {
    __shared__ int red[4];
    __shared__ int wave_kept[4];
    const int tid = threadIdx.x, chunk = blockIdx.x, lane = tid & 63, wv = tid >> 6;
    if (chunk == 0) {                                                       // the per-image counts: the image's chunks in index order
        for (int k = tid; k < n_images; k += BL_THREADS) {
            const umr_bl_image e = images[k];
            const int nc = e.R > 0 ? (e.R + BL_THREADS - 1) / BL_THREADS : 0;
            int s = 0;
            for (int c = 0; c < nc && e.chunk_first >= 0 && e.chunk_first + c < n_chunks; ++c) s += chunk_counts[e.chunk_first + c];
            counts[k] = s;
        }
    }
    int before = 0;
    for (int c = tid; c < chunk; c += BL_THREADS) before += chunk_counts[c];
    const int base = bl_block_sum(before, red);
    const umr_bl_image im = images[bl_find(images, n_images, chunk)];
    if (!bl_entry_ok(im, chunk, R)) return;
    const int j = (chunk - im.chunk_first) * BL_THREADS + tid;
    const int64_t r = (int64_t)im.first + j;
    const bool kept = j < im.R && keep[r];
    const unsigned long long vote = __ballot(kept);
    const int in_wave = __popcll(vote & ((1ull << lane) - 1ull));
    if (lane == 0) wave_kept[wv] = __popcll(vote);
    __syncthreads();
    int off = base + in_wave;
    for (int w = 0; w < wv; ++w) off += wave_kept[w];
    if (kept && off < R) {                                                  // off < R always: at most R rows are kept
        const float* s = tmp + r * 4;
        float* d = out + (int64_t)off * 4;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
    }
}

template <typename T>
__global__ __launch_bounds__(BL_THREADS) void bl_apply_kernel(const T* __restrict__ deltas, const float* __restrict__ boxes, int64_t n,
                                                              BlW bw, float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * BL_THREADS + threadIdx.x;
    if (r >= n) return;
    const float box[4] = {boxes[r * 4], boxes[r * 4 + 1], boxes[r * 4 + 2], boxes[r * 4 + 3]};
    const float d[4] = {to_f32<T>(deltas[r * 4]), to_f32<T>(deltas[r * 4 + 1]), to_f32<T>(deltas[r * 4 + 2]), to_f32<T>(deltas[r * 4 + 3])};
    float o[4];
    box_apply_deltas(d, box, bw.v, o);
    out[r * 4] = o[0]; out[r * 4 + 1] = o[1]; out[r * 4 + 2] = o[2]; out[r * 4 + 3] = o[3];
}

__global__ __launch_bounds__(BL_THREADS) void bl_get_kernel(const float* __restrict__ src, const float* __restrict__ target, int64_t n, BlW bw,
                                                            float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * BL_THREADS + threadIdx.x;
    if (r >= n) return;
    const float s[4] = {src[r * 4], src[r * 4 + 1], src[r * 4 + 2], src[r * 4 + 3]};
    const float t[4] = {target[r * 4], target[r * 4 + 1], target[r * 4 + 2], target[r * 4 + 3]};
    float o[4];
    (void)box_get_deltas(s, t, bw.v, o);                                    // the plain op returns what the arithmetic gives, NaN and inf included
    out[r * 4] = o[0]; out[r * 4 + 1] = o[1]; out[r * 4 + 2] = o[2]; out[r * 4 + 3] = o[3];
}

// ---------------------------------------------------------------------------------------------------------------- weights and losses
// drop_mode: 0 = weights of one, 1 = weights_in, 2 = the drop-loss rule
template <typename T, bool LOSS>
__global__ __launch_bounds__(BL_THREADS) void bl_loss_kernel(const umr_bl_image* __restrict__ images, int n_images, int R, int K1,
                                                             long long num_classes, const T* __restrict__ scores, const T* __restrict__ deltas,
                                                             BlW bw, float beta, int soft, int drop_mode, float iou_thresh,
                                                             const float* __restrict__ weights_in, const float* __restrict__ single,
                                                             float* __restrict__ weights_out, T* __restrict__ grad_scores,
                                                             T* __restrict__ grad_deltas, Partial* __restrict__ partials) {
    __shared__ float set[BL_UNIQUE_ROWS][5];                               // the image's first rows of matched gt_boxes, with their areas
    __shared__ int red[4];
    __shared__ double red_d[8];
    __shared__ long long red_n[28];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const umr_bl_image im = images[bl_find(images, n_images, chunk)];
    const bool need_gt = LOSS || drop_mode == 2;
    if (!bl_entry_ok(im, chunk, R) || (need_gt && !im.gt_boxes) || (LOSS && !(im.gt_classes && (!soft || im.gt_scores)))) {
        if (LOSS && tid == 0) partials[chunk] = Partial{};
        return;
    }
    // ---- the drop-loss ground-truth set: the first n_set rows, n_set = the number of DISTINCT rows among the first min(100, R_i)
    int n_set = 0;
    if (drop_mode == 2) {
        const int m = min(BL_UNIQUE_ROWS, im.R);
        if (tid < m) {
            const float* b = im.gt_boxes + (int64_t)tid * 4;
            set[tid][0] = b[0]; set[tid][1] = b[1]; set[tid][2] = b[2]; set[tid][3] = b[3];
            set[tid][4] = box_area(b[0], b[1], b[2], b[3]);
        }
        __syncthreads();
        int first_of_its_kind = 0;
        if (tid < m) {
            first_of_its_kind = 1;
            for (int q = 0; q < tid; ++q)
                if (set[q][0] == set[tid][0] && set[q][1] == set[tid][1] && set[q][2] == set[tid][2] && set[q][3] == set[tid][3]) {
                    first_of_its_kind = 0;
                    break;
                }
        }
        n_set = bl_block_sum(first_of_its_kind, red);
    }

    const int j = (chunk - im.chunk_first) * BL_THREADS + tid;
    double sums[2] = {0.0, 0.0};
    long long n[7] = {0, 0, 0, 0, 0, 0, 0};
    if (j < im.R) {
        const int64_t r = (int64_t)im.first + j;
        const float* b = im.boxes + (int64_t)j * 4;
        const float box[4] = {b[0], b[1], b[2], b[3]};
        const float d[4] = {to_f32<T>(deltas[r * 4]), to_f32<T>(deltas[r * 4 + 1]), to_f32<T>(deltas[r * 4 + 2]), to_f32<T>(deltas[r * 4 + 3])};
        // ---- the row's weight
        float w = 1.f;
        if (drop_mode == 1) {
            w = weights_in[r];
        } else if (drop_mode == 2) {
            float o[4];
            box_apply_deltas(d, box, bw.v, o);                              // the stage's own prediction, unclipped
            const float o_area = box_area(o[0], o[1], o[2], o[3]);
            float iou_max = -1.f;
            for (int g = 0; g < n_set; ++g) {
                const float v = box_iou_match(o[0], o[1], o[2], o[3], o_area, set[g][0], set[g][1], set[g][2], set[g][3], set[g][4]);
                if (v > iou_max || v != v) iou_max = v;                     // torch.max: a NaN wins and stays
            }
            w = (iou_max <= iou_thresh) ? 0.f : 1.f;                        // 1 - (iou_max <= thresh): a NaN keeps the row
            const int per_image = R / n_images;                            // the reference's indicator BY POSITION, not by image
            if (single && per_image > 0) {
                const int64_t i = r / per_image;
                if (i < n_images && single[i] == 1.f) w = 1.f;
            }
        }
        weights_out[r] = w;
        if constexpr (LOSS) {
            const long long gc = im.gt_classes[j];
            const bool fg = gc >= 0 && gc < num_classes;
            const float score = soft ? im.gt_scores[j] : 1.f;
            bool bad = false;
            // ---- cross-entropy: log-softmax over the row in float32
            const T* x = scores + r * K1;
            float mx = to_f32<T>(x[0]);
            int arg = 0;
            for (int c = 1; c < K1; ++c) {
                const float v = to_f32<T>(x[c]);
                if (v > mx) { mx = v; arg = c; }
            }
            float S = 0.f;
            for (int c = 0; c < K1; ++c) S += expf(to_f32<T>(x[c]) - mx);
            const float log_s = logf(S);
            float ce = 0.f;
            const float fgp = (soft && gc != num_classes) ? score : 0.f;    // soft targets: (fgp, 1 - fgp), K1 == 2
            const bool hard_ok = gc >= 0 && gc < K1;
            if (soft) {
                const float lp0 = (to_f32<T>(x[0]) - mx) - log_s, lp1 = (to_f32<T>(x[1]) - mx) - log_s;
                ce = -(fgp * lp0 + (1.f - fgp) * lp1);
            } else if (hard_ok) {
                ce = -((to_f32<T>(x[gc]) - mx) - log_s);
            } else {
                bad = true;                                                 // a class no column stands for: no loss, no gradient
            }
            sums[0] = (double)(w * ce);
            // softmax - target without the cancellation of p - 1: with p0 + p1 = 1, p0 - fg = p0 (1 - fg) - p1 fg, and the other column is
            // its negative; for a class target, p - 1 = -(the others' share)
            if (soft) {
                const float p0 = __fdiv_rn(expf(to_f32<T>(x[0]) - mx), S), p1 = __fdiv_rn(expf(to_f32<T>(x[1]) - mx), S);
                const float g = __fdiv_rn(w * (p0 * (1.f - fgp) - p1 * fgp), (float)R);
                grad_scores[r * 2] = from_f32<T>(g);
                grad_scores[r * 2 + 1] = from_f32<T>(-g);
            } else {
                float others = 0.f;
                for (int c = 0; c < K1; ++c)
                    if (c != gc) others += expf(to_f32<T>(x[c]) - mx);
                for (int c = 0; c < K1; ++c) {
                    float g = 0.f;
                    if (hard_ok) {
                        const float pc = c == gc ? -__fdiv_rn(others, S) : __fdiv_rn(expf(to_f32<T>(x[c]) - mx), S);
                        g = __fdiv_rn(w * pc, (float)R);
                    }
                    grad_scores[r * K1 + c] = from_f32<T>(g);
                }
            }
            // ---- box regression on the foreground rows
            float gd[4] = {0.f, 0.f, 0.f, 0.f};
            if (fg) {
                const float* gb = im.gt_boxes + (int64_t)j * 4;
                const float tb[4] = {gb[0], gb[1], gb[2], gb[3]};
                float t[4];
                const bool ok = box_get_deltas(box, tb, bw.v, t) && box_finite(score);
                if (ok) {
                    float row = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float e = d[c] - t[c], a = fabsf(e);
                        float l, g;
                        if (beta < 1e-5f) {
                            l = a;
                            g = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
                        } else if (a < beta) {
                            l = __fdiv_rn(.5f * e * e, beta);
                            g = __fdiv_rn(e, beta);
                        } else {
                            l = a - .5f * beta;
                            g = e > 0.f ? 1.f : -1.f;
                        }
                        row += l * score;
                        gd[c] = __fdiv_rn(g * score, (float)R);
                    }
                    sums[1] = (double)row;
                } else {
                    bad = true;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) grad_deltas[r * 4 + c] = from_f32<T>(gd[c]);
            n[0] = 1; n[1] = fg; n[2] = arg == gc; n[3] = fg && arg == gc; n[4] = fg && arg == K1 - 1; n[5] = w == 0.f; n[6] = bad;
        }
    }
    if constexpr (LOSS) {
        block_sum_fixed(sums, n, red_d, red_n);
        if (tid == 0) {
            Partial q;
            q.d[0] = sums[0];
            q.d[1] = sums[1];
#pragma unroll
            for (int c = 0; c < 7; ++c) q.c[c] = (int32_t)n[c];
            q.c[7] = 0;
            partials[chunk] = q;
        }
    }
}

__global__ __launch_bounds__(BL_THREADS) void bl_finish_kernel(const Partial* __restrict__ partials, int n_partials, double rows,
                                                               float* __restrict__ loss_cls, float* __restrict__ loss_box,
                                                               int64_t* __restrict__ counters) {
    __shared__ double red_d[8];
    __shared__ long long red_n[28];
    double d[2];
    long long n[7];
    partials_sum_fixed(partials, n_partials, d, n, red_d, red_n);
    if (threadIdx.x == 0) {
        loss_cls[0] = rows > 0 ? (float)(d[0] / rows) : 0.f;               // the mean over R
        loss_box[0] = (float)(d[1] / (rows > 1.0 ? rows : 1.0));            // / max(R, 1)
#pragma unroll
        for (int k = 0; k < 7; ++k) counters[k] = n[k];
    }
}

int bl_check_table(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks) {
    UMR_CHECK_ARG(n_images >= 0 && R >= 0 && n_chunks >= 0, "box_loss: negative extent");
    UMR_CHECK_ARG(R <= INT_MAX && n_chunks <= INT_MAX, "box_loss: more than 2^31 - 1 proposals");
    UMR_CHECK_ARG(n_chunks <= R && (R == 0 || n_chunks >= (R + BL_THREADS - 1) / BL_THREADS),
                  "box_loss: n_chunks must be the sum over the images of ceil(R_i / 256)");
    UMR_CHECK_ARG(R == 0 || (images && n_images > 0), "box_loss: proposals without an image table");
    return UMR_OK;
}

int bl_check_weights(float wx, float wy, float ww, float wh, BlW* out) {
    UMR_CHECK_ARG(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f && wx <= FLT_MAX && wy <= FLT_MAX && ww <= FLT_MAX && wh <= FLT_MAX,
                  "box_loss: the box2box weights must be positive and finite");
    *out = BlW{{wx, wy, ww, wh}};
    return UMR_OK;
}

}  // namespace

extern "C" int64_t umr_box_loss_workspace(int64_t n_chunks) {
    if (n_chunks < 0 || n_chunks > INT_MAX) return -1;
    return std::max<int64_t>(n_chunks, 1) * (int64_t)sizeof(Partial);
}

extern "C" int64_t umr_box_decode_workspace(int64_t R, int64_t n_chunks) {
    if (R < 0 || n_chunks < 0 || R > INT_MAX || n_chunks > INT_MAX) return -1;
    return std::max<int64_t>(R, 1) * 16 + std::max<int64_t>(n_chunks, 1) * 4;
}

extern "C" int umr_box_match(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, float iou_threshold, int64_t num_classes,
                             int64_t* matched_idxs, float* matched_vals, int64_t* gt_classes, float* gt_boxes, float* gt_scores,
                             int32_t* counts, umr_stream_t stream) {
    if (int st = bl_check_table(images, n_images, R, n_chunks)) return st;
    UMR_CHECK_ARG(num_classes >= 0, "box_loss: negative num_classes");
    UMR_CHECK_ARG(iou_threshold == iou_threshold, "box_loss: the IoU threshold is NaN");
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(matched_idxs && matched_vals && gt_classes && gt_boxes && gt_scores && counts, "box_loss: null output");
    bl_match_kernel<<<(int)n_chunks, BL_THREADS, 0, (hipStream_t)stream>>>(images, n_images, (int)R, iou_threshold, (long long)num_classes,
                                                                        matched_idxs, matched_vals, gt_classes, gt_boxes, gt_scores, counts);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_box_decode(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, const void* deltas, int dtype, float wx,
                              float wy, float ww, float wh, int training, float* boxes, uint8_t* keep, int32_t* counts, void* workspace,
                              int64_t workspace_bytes, umr_stream_t stream) {
    if (int st = bl_check_table(images, n_images, R, n_chunks)) return st;
    BlW bw;
    if (int st = bl_check_weights(wx, wy, ww, wh, &bw)) return st;
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "box_loss: deltas must be UMR_F32 or UMR_BF16");
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(deltas && boxes && keep && counts && workspace, "box_loss: null pointer");
    UMR_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "box_loss: workspace not 4-byte aligned");
    UMR_CHECK_ARG(workspace_bytes >= umr_box_decode_workspace(R, n_chunks), "box_loss: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float* tmp = (float*)workspace;
    int32_t* chunk_counts = (int32_t*)(tmp + R * 4);
    if (dtype == UMR_F32)
        bl_decode_kernel<float><<<(int)n_chunks, BL_THREADS, 0, s>>>(images, n_images, (int)R, (const float*)deltas, bw, training, tmp, keep,
                                                                    chunk_counts);
    else
        bl_decode_kernel<bf16_t><<<(int)n_chunks, BL_THREADS, 0, s>>>(images, n_images, (int)R, (const bf16_t*)deltas, bw, training, tmp, keep,
                                                                     chunk_counts);
    UMR_LAUNCH_CHECK();
    bl_compact_kernel<<<(int)n_chunks, BL_THREADS, 0, s>>>(images, n_images, (int)R, (int)n_chunks, tmp, keep, chunk_counts, boxes, counts);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_box_apply_deltas(const void* deltas, int dtype, const float* boxes, int64_t n, float wx, float wy, float ww, float wh,
                                    float* out, umr_stream_t stream) {
    BlW bw;
    if (int st = bl_check_weights(wx, wy, ww, wh, &bw)) return st;
    UMR_CHECK_ARG(n >= 0 && n <= INT_MAX, "box_loss: the number of boxes must be in [0, 2^31)");
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "box_loss: deltas must be UMR_F32 or UMR_BF16");
    if (n == 0) return UMR_OK;
    UMR_CHECK_ARG(deltas && boxes && out, "box_loss: null pointer");
    const int grid = (int)((n + BL_THREADS - 1) / BL_THREADS);
    if (dtype == UMR_F32)
        bl_apply_kernel<float><<<grid, BL_THREADS, 0, (hipStream_t)stream>>>((const float*)deltas, boxes, n, bw, out);
    else
        bl_apply_kernel<bf16_t><<<grid, BL_THREADS, 0, (hipStream_t)stream>>>((const bf16_t*)deltas, boxes, n, bw, out);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_box_get_deltas(const float* src, const float* target, int64_t n, float wx, float wy, float ww, float wh, float* out,
                                  umr_stream_t stream) {
    BlW bw;
    if (int st = bl_check_weights(wx, wy, ww, wh, &bw)) return st;
    UMR_CHECK_ARG(n >= 0 && n <= INT_MAX, "box_loss: the number of boxes must be in [0, 2^31)");
    if (n == 0) return UMR_OK;
    UMR_CHECK_ARG(src && target && out, "box_loss: null pointer");
    bl_get_kernel<<<(int)((n + BL_THREADS - 1) / BL_THREADS), BL_THREADS, 0, (hipStream_t)stream>>>(src, target, n, bw, out);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_box_drop_weights(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, const void* deltas, int dtype,
                                    float wx, float wy, float ww, float wh, float iou_thresh, const float* is_single_object, float* weights,
                                    umr_stream_t stream) {
    if (int st = bl_check_table(images, n_images, R, n_chunks)) return st;
    BlW bw;
    if (int st = bl_check_weights(wx, wy, ww, wh, &bw)) return st;
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "box_loss: deltas must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(iou_thresh == iou_thresh, "box_loss: the IoU threshold is NaN");
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(deltas && weights, "box_loss: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == UMR_F32)
        bl_loss_kernel<float, false><<<(int)n_chunks, BL_THREADS, 0, s>>>(images, n_images, (int)R, 0, 0, nullptr, (const float*)deltas, bw, 0.f, 0, 2,
                                                                         iou_thresh, nullptr, is_single_object, weights, nullptr, nullptr,
                                                                         nullptr);
    else
        bl_loss_kernel<bf16_t, false><<<(int)n_chunks, BL_THREADS, 0, s>>>(images, n_images, (int)R, 0, 0, nullptr, (const bf16_t*)deltas, bw, 0.f, 0,
                                                                          2, iou_thresh, nullptr, is_single_object, weights, nullptr, nullptr,
                                                                          nullptr);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_box_loss(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, int K1, int64_t num_classes,
                            const void* scores, const void* deltas, int dtype, float wx, float wy, float ww, float wh, float smooth_l1_beta,
                            int soft_targets, int drop_mode, float iou_thresh, const float* weights_in, const float* is_single_object,
                            int phases, float* weights, void* grad_scores, void* grad_deltas, float* loss_cls, float* loss_box_reg,
                            int64_t* counters, void* workspace, int64_t workspace_bytes, umr_stream_t stream) {
    if (int st = bl_check_table(images, n_images, R, n_chunks)) return st;
    BlW bw;
    if (int st = bl_check_weights(wx, wy, ww, wh, &bw)) return st;
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "box_loss: scores and deltas must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(num_classes >= 1 && num_classes < INT_MAX && K1 == (int)num_classes + 1, "box_loss: the scores need num_classes + 1 columns");
    UMR_CHECK_ARG(!soft_targets || K1 == 2, "box_loss: soft targets need exactly two columns (foreground, background)");
    UMR_CHECK_ARG(smooth_l1_beta >= 0.f, "box_loss: smooth_l1_beta must be >= 0");
    UMR_CHECK_ARG(drop_mode >= 0 && drop_mode <= 2, "box_loss: drop_mode is 0 (none), 1 (weights given) or 2 (the drop-loss rule)");
    UMR_CHECK_ARG(drop_mode != 1 || R == 0 || weights_in, "box_loss: drop_mode 1 needs weights");
    UMR_CHECK_ARG(iou_thresh == iou_thresh, "box_loss: the IoU threshold is NaN");
    UMR_CHECK_ARG(phases > 0 && phases < 4, "box_loss: phases is a mask of 1 (weights, loss terms, gradients), 2 (finish)");
    UMR_CHECK_ARG(loss_cls && loss_box_reg && counters && workspace, "box_loss: null pointer");
    UMR_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "box_loss: workspace not 8-byte aligned");
    UMR_CHECK_ARG(workspace_bytes >= umr_box_loss_workspace(n_chunks), "box_loss: workspace too small");
    UMR_CHECK_ARG(R == 0 || (scores && deltas && weights && grad_scores && grad_deltas), "box_loss: null scores, deltas, weights or gradient");
    hipStream_t s = (hipStream_t)stream;
    Partial* partials = (Partial*)workspace;
    if ((phases & 1) && R > 0) {
        if (dtype == UMR_F32)
            bl_loss_kernel<float, true><<<(int)n_chunks, BL_THREADS, 0, s>>>(images, n_images, (int)R, K1, (long long)num_classes,
                                                                            (const float*)scores, (const float*)deltas, bw, smooth_l1_beta,
                                                                            soft_targets, drop_mode, iou_thresh, weights_in, is_single_object,
                                                                            weights, (float*)grad_scores, (float*)grad_deltas, partials);
        else
            bl_loss_kernel<bf16_t, true><<<(int)n_chunks, BL_THREADS, 0, s>>>(images, n_images, (int)R, K1, (long long)num_classes,
                                                                             (const bf16_t*)scores, (const bf16_t*)deltas, bw, smooth_l1_beta,
                                                                             soft_targets, drop_mode, iou_thresh, weights_in, is_single_object,
                                                                             weights, (bf16_t*)grad_scores, (bf16_t*)grad_deltas, partials);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        bl_finish_kernel<<<1, BL_THREADS, 0, s>>>(partials, R > 0 ? (int)n_chunks : 0, (double)R, loss_cls, loss_box_reg, counters);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
