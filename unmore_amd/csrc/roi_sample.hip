// The first step of the stage-3 detector's cascade ROI heads in training (cad/modeling/roi_heads/roi_heads.py:207-328, Detectron2's
// ROIHeads.label_and_sample_proposals with _sample_proposals, subsample_labels and add_ground_truth_to_proposals): the image's ground
// truths are appended to its RPN proposals, every candidate is matched to the image's ground truths and labelled, a batch of candidates
// per image is sampled, ordered, and every field of the samples is gathered.  Two launches for the whole batch; no [G, R] matrix, no
// concatenated copy of proposals and ground truths, no atomics on memory at all (counts are workgroup sums, one workgroup per image), so
// the same input gives the same bytes; nothing is read back and nothing is allocated.
//
// The table (include/umr.h: RS_FIELDS int64 per image, on the device) names the image's sources; candidate r of image n is proposal r for
// r < R and ground truth r - R for R <= r < R + A (A = G with the append, else 0); C = R + A <= 16384.  The candidates of all images lie
// one after the other in the per-candidate arrays, image n's at cand_first; they are cut into chunks of 256 per image (chunk_first).
//   rs_match_kernel    a workgroup per chunk, found by bisection on chunk_first as box_loss.hip's bl_find does; a thread per candidate;
//                      the image's ground truths pass through LDS in tiles of 256 with their areas.  Per candidate the maximum IoU and the
//                      LOWEST index that attains it (`>`; a NaN never wins), foreground iff maximum >= threshold; the pool of
//                      subsample_labels from the class (positive: class != -1 and != num_classes; negative: class == num_classes); a
//                      candidate with a non-finite coordinate is in no pool (`bad`).  It leaves matched index, value, pool and key.
//   rs_select_kernel   one workgroup of 1024 threads per image: P, Q and bad by a workgroup sum; num_pos = min(P, pos_cap), num_neg =
//                      min(Q, B - num_pos); select_in_order.h's radix select twice (the positives' keys, then the negatives'; the other
//                      pool has key 0), which leaves each part in ascending r; for order "key" a rank sort of each part in LDS by (key
//                      descending, r ascending); then the gathers, coalesced over (row, field), and the rows past the count: zero, class -1.
//
// Key of candidate r of image n (31 bits, 0 mapped to 1 so that 0 can mean "not in this pool"): keys[r] & 0x7fffffff when the image has
// keys, else det_box.h's sample_key: fmix(fmix(r ^ s_lo) ^ (n * 0x9e3779b9 + s_hi)) >> 1 with murmur3's 32-bit finaliser and the halves of
// the (salted, by the caller) seed.  IoU: det_box.h's box_iou_match, float32, no contraction, every operation rounded on its own.
#pragma clang fp contract(off)
#include "umr_common.h"
#include "det_box.h"
#include "select_in_order.h"
#include <algorithm>
#include <float.h>
#include <limits.h>

namespace {

constexpr int RS_FIELDS = 11;                         // int64 per image, see include/umr.h
constexpr int RS_THREADS = 256;                       // candidates per chunk
constexpr int RS_GT_TILE = 256;                       // == RS_THREADS: one load per thread
constexpr int RS_SELECT_THREADS = 1024;
constexpr int RS_MAX_BATCH = 1024;
constexpr int RS_MAX_CANDIDATES = 16384;              // select_in_order in one step
constexpr int RS_COUNTERS = 5;                        // P, Q, sampled foreground, sampled background, bad candidates
constexpr int RS_POOL_NEG = 0, RS_POOL_POS = 1, RS_POOL_NONE = 2, RS_FG = 4, RS_BAD = 8;   // info = pool | RS_FG (foreground) | RS_BAD

struct RsImage {
    const float* boxes;               // [R,4] proposals
    const float* logits;              // [R]
    const float* gt_boxes;            // [G,4]
    const int64_t* gt_classes;        // [G]
    const float* gt_scores;           // [G] or NULL
    const int32_t* keys;              // [C] or NULL: the hash
    int R, G, A, chunk_first, cand_first;
    __device__ __forceinline__ int C() const { return R + A; }
};

__device__ __forceinline__ RsImage rs_load(const int64_t* __restrict__ table, int n) {
    const int64_t* e = table + (int64_t)n * RS_FIELDS;
    RsImage im;
    im.boxes = (const float*)(uintptr_t)e[0];
    im.logits = (const float*)(uintptr_t)e[1];
    im.gt_boxes = (const float*)(uintptr_t)e[2];
    im.gt_classes = (const int64_t*)(uintptr_t)e[3];
    im.gt_scores = (const float*)(uintptr_t)e[4];
    im.keys = (const int32_t*)(uintptr_t)e[5];
    im.R = (int)e[6]; im.G = (int)e[7]; im.A = (int)e[8]; im.chunk_first = (int)e[9]; im.cand_first = (int)e[10];
    return im;
}

// what the kernels trust of a table entry before they index with it
__device__ __forceinline__ bool rs_entry_ok(const RsImage& im, int n_cand) {
    return im.R >= 0 && im.G >= 0 && (im.A == 0 || im.A == im.G) && im.R <= RS_MAX_CANDIDATES && im.A <= RS_MAX_CANDIDATES &&
           im.C() <= RS_MAX_CANDIDATES && im.cand_first >= 0 && im.cand_first <= n_cand - im.C() && im.chunk_first >= 0 &&
           (im.R == 0 || (im.boxes && im.logits)) && (im.G == 0 || (im.gt_boxes && im.gt_classes));
}

__device__ __forceinline__ int rs_find(const int64_t* __restrict__ table, int n_images, int chunk) {
    int lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)table[(int64_t)mid * RS_FIELDS + 9] <= chunk) lo = mid; else hi = mid;
    }
    return lo;
}

// candidate r of the image: a proposal, or an appended ground truth
__device__ __forceinline__ const float* rs_candidate(const RsImage& im, int r) {
    return r < im.R ? im.boxes + (int64_t)r * 4 : im.gt_boxes + (int64_t)(r - im.R) * 4;
}

// ---------------------------------------------------------------------------------------------------------------- match
__global__ __launch_bounds__(RS_THREADS) void rs_match_kernel(const int64_t* __restrict__ table, int n_images, int n_cand, float threshold,
                                                              long long num_classes, unsigned s_lo, unsigned s_hi,
                                                              int32_t* __restrict__ midx, float* __restrict__ mval,
                                                              int32_t* __restrict__ info, uint32_t* __restrict__ ckey) {
    __shared__ float gt[RS_GT_TILE][5];                                   // x1 y1 x2 y2 area
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const int n = rs_find(table, n_images, chunk);
    const RsImage im = rs_load(table, n);
    if (!rs_entry_ok(im, n_cand) || chunk < im.chunk_first || (int64_t)(chunk - im.chunk_first) * RS_THREADS >= im.C()) return;   // uniform
    const int r = (chunk - im.chunk_first) * RS_THREADS + tid;
    const bool live = r < im.C();
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        const float* b = rs_candidate(im, r);
        p[0] = b[0]; p[1] = b[1]; p[2] = b[2]; p[3] = b[3];
    }
    const bool bad = live && !(box_finite(p[0]) && box_finite(p[1]) && box_finite(p[2]) && box_finite(p[3]));
    const float p_area = box_area(p[0], p[1], p[2], p[3]);
    float best = -1.f;
    int best_g = 0;
    for (int g0 = 0; g0 < im.G; g0 += RS_GT_TILE) {
        const int cnt = min(RS_GT_TILE, im.G - g0);
        __syncthreads();
        if (tid < cnt) {
            const float* b = im.gt_boxes + (int64_t)(g0 + tid) * 4;
            gt[tid][0] = b[0]; gt[tid][1] = b[1]; gt[tid][2] = b[2]; gt[tid][3] = b[3];
            gt[tid][4] = box_area(b[0], b[1], b[2], b[3]);
        }
        __syncthreads();
        if (live && !bad) {
            for (int g = 0; g < cnt; ++g) {
                const float v = box_iou_match(gt[g][0], gt[g][1], gt[g][2], gt[g][3], gt[g][4], p[0], p[1], p[2], p[3], p_area);
                if (v > best) { best = v; best_g = g0 + g; }              // strict: the lowest index that attains the maximum; a NaN never wins
            }
        }
    }
    if (!live) return;
    const bool matched = !bad && im.G > 0 && best >= 0.f;
    const bool fg = matched && best >= threshold;
    if (!matched) best_g = 0;
    int pool = RS_POOL_NEG;                                               // background: class == num_classes
    if (bad) {
        pool = RS_POOL_NONE;
    } else if (fg) {
        const long long c = im.gt_classes[best_g];
        pool = (c != -1 && c != num_classes) ? RS_POOL_POS : (c == num_classes ? RS_POOL_NEG : RS_POOL_NONE);
    }
    unsigned k = im.keys ? (unsigned)im.keys[r] : sample_key((unsigned)r, (unsigned)n, s_lo, s_hi);
    k &= 0x7fffffffu;
    const int64_t at = (int64_t)im.cand_first + r;
    midx[at] = best_g;
    mval[at] = matched ? best : 0.f;
    info[at] = pool | (fg ? RS_FG : 0) | (bad ? RS_BAD : 0);
    ckey[at] = k ? k : 1u;
}

// ---------------------------------------------------------------------------------------------------------------- select, order, gather
// the keys of one pool of an image's candidates: 0 for a candidate of another pool
struct RsKeys {
    const int32_t* info; const uint32_t* ckey; int want;
    __device__ __forceinline__ unsigned key(int64_t i) const { return (info[i] & 3) == want ? ckey[i] : 0u; }
};

__global__ __launch_bounds__(RS_SELECT_THREADS) void rs_select_kernel(const int64_t* __restrict__ table, int n_cand, int B, int pos_cap,
                                                                      int by_key, long long num_classes, float gt_logit,
                                                                      const int32_t* __restrict__ midx, const int32_t* __restrict__ info,
                                                                      const uint32_t* __restrict__ ckey, float* __restrict__ out_boxes,
                                                                      float* __restrict__ out_logits, int64_t* __restrict__ out_classes,
                                                                      float* __restrict__ out_gt_boxes, float* __restrict__ out_gt_scores,
                                                                      int64_t* __restrict__ out_midx, int32_t* __restrict__ out_sampled,
                                                                      int32_t* __restrict__ counts, int32_t* __restrict__ counters) {
    __shared__ int hist[256];
    __shared__ int wtot[32];
    __shared__ int32_t picked[RS_MAX_BATCH];
    __shared__ int32_t sorted[RS_MAX_BATCH];
    __shared__ uint32_t skey[RS_MAX_BATCH];
    __shared__ int s_cnt[3];
    const int n = blockIdx.x, tid = threadIdx.x;
    RsImage im = rs_load(table, n);
    if (!rs_entry_ok(im, n_cand)) { im.R = im.G = im.A = 0; im.cand_first = 0; }      // workgroup-uniform: an image without candidates
    const int C = im.C();
    const int32_t* my_info = info + im.cand_first;
    const uint32_t* my_key = ckey + im.cand_first;
    const int32_t* my_midx = midx + im.cand_first;
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    for (int base = 0; base < C; base += RS_SELECT_THREADS) {
        const int i = base + tid;
        const int v = i < C ? my_info[i] : RS_POOL_NONE;
        const unsigned long long vp = __ballot((v & 3) == RS_POOL_POS), vn = __ballot((v & 3) == RS_POOL_NEG), vb = __ballot((v & RS_BAD) != 0);
        if ((tid & 63) == 0) {
            if (vp) atomicAdd(&s_cnt[0], __popcll(vp));
            if (vn) atomicAdd(&s_cnt[1], __popcll(vn));
            if (vb) atomicAdd(&s_cnt[2], __popcll(vb));
        }
    }
    __syncthreads();
    const int P = s_cnt[0], Q = s_cnt[1], n_bad = s_cnt[2];
    const int num_pos = min(P, pos_cap), num_neg = min(Q, B - num_pos), S = num_pos + num_neg;
    const RsKeys pos_keys{my_info, my_key, RS_POOL_POS}, neg_keys{my_info, my_key, RS_POOL_NEG};
    if (num_pos > 0) (void)select_in_order(pos_keys, (int64_t)C, num_pos, hist, wtot, SelectStoreIndex{picked});
    if (num_neg > 0) (void)select_in_order(neg_keys, (int64_t)C, num_neg, hist, wtot, SelectStoreIndex{picked + num_pos});
    __syncthreads();
    if (by_key) {
        // each part is in ascending r: among equal keys the lower r is the lower position
        if (tid < S) skey[tid] = my_key[min(max(picked[tid], 0), max(C - 1, 0))];
        __syncthreads();
        if (tid < S) {
            const int lo = tid < num_pos ? 0 : num_pos, hi = tid < num_pos ? num_pos : S;
            const uint32_t mine = skey[tid];
            int rank = lo;
            for (int j = lo; j < hi; ++j) rank += (skey[j] > mine || (skey[j] == mine && j < tid)) ? 1 : 0;
            sorted[rank] = picked[tid];
        }
    } else if (tid < S) {
        sorted[tid] = picked[tid];
    }
    __syncthreads();
    // ---- the gathers: (row, coordinate) for the boxes, a row per thread for the rest
    const int64_t row0 = (int64_t)n * B;
    for (int e = tid; e < B * 4; e += RS_SELECT_THREADS) {
        const int s = e >> 2, f = e & 3;
        float box = 0.f, gbox = 0.f;
        if (s < S) {
            const int r = min(max(sorted[s], 0), C - 1);                  // always inside: the indices are this launch's own
            box = rs_candidate(im, r)[f];
            if (im.G > 0) gbox = im.gt_boxes[(int64_t)min(max(my_midx[r], 0), im.G - 1) * 4 + f];
        }
        out_boxes[row0 * 4 + e] = box;
        out_gt_boxes[row0 * 4 + e] = gbox;
    }
    for (int s = tid; s < B; s += RS_SELECT_THREADS) {
        float logit = 0.f, score = 0.f;
        long long cls = -1;
        int g = 0, r = 0;
        if (s < S) {
            r = min(max(sorted[s], 0), C - 1);
            logit = r < im.R ? im.logits[r] : gt_logit;
            cls = num_classes;
            if (im.G > 0) {
                g = min(max(my_midx[r], 0), im.G - 1);
                if (my_info[r] & RS_FG) cls = im.gt_classes[g];
                if (im.gt_scores) score = im.gt_scores[g];
            }
        }
        out_logits[row0 + s] = logit;
        out_classes[row0 + s] = cls;
        if (out_gt_scores) out_gt_scores[row0 + s] = score;
        out_midx[row0 + s] = g;
        out_sampled[row0 + s] = r;
    }
    if (tid == 0) {
        counts[n * 2] = num_pos;
        counts[n * 2 + 1] = num_neg;
        int32_t* c = counters + n * RS_COUNTERS;
        c[0] = P; c[1] = Q; c[2] = num_pos; c[3] = num_neg; c[4] = n_bad;
    }
}

}  // namespace

extern "C" int64_t umr_roi_sample_workspace(int64_t n_cand) {
    if (n_cand < 0 || n_cand > (int64_t)65535 * RS_MAX_CANDIDATES) return -1;
    return std::max<int64_t>(n_cand, 1) * 16;                             // matched index, value, info, key: 4 bytes each per candidate
}

extern "C" int umr_roi_sample(const int64_t* table, int n_images, int64_t n_cand, int64_t n_chunks, float iou_threshold,
                              int64_t num_classes, int batch_size, int pos_cap, int by_key, float gt_logit, int64_t seed, int phases,
                              float* out_boxes, float* out_logits, int64_t* out_classes, float* out_gt_boxes, float* out_gt_scores,
                              int64_t* out_matched_idxs, int32_t* out_sampled_idxs, int32_t* counts, int32_t* counters, void* workspace,
                              int64_t workspace_bytes, umr_stream_t stream) {
    UMR_CHECK_ARG(table && n_images >= 1 && n_images <= 65535, "roi_sample: the table of between 1 and 65535 images on the device");
    UMR_CHECK_ARG(n_cand >= 0 && n_cand <= (int64_t)n_images * RS_MAX_CANDIDATES && n_cand < INT_MAX,
                  "roi_sample: at most 16384 candidates per image and fewer than 2^31 in all");
    UMR_CHECK_ARG(n_chunks >= 0 && n_chunks <= n_cand && n_chunks * RS_THREADS >= n_cand, "roi_sample: n_chunks does not fit n_cand");
    UMR_CHECK_ARG(iou_threshold == iou_threshold, "roi_sample: the IoU threshold is NaN");
    UMR_CHECK_ARG(batch_size >= 1 && batch_size <= RS_MAX_BATCH && pos_cap >= 0 && pos_cap <= batch_size,
                  "roi_sample: 1 <= batch_size <= 1024 and 0 <= pos_cap <= batch_size");
    UMR_CHECK_ARG(out_boxes && out_logits && out_classes && out_gt_boxes && out_matched_idxs && out_sampled_idxs && counts && counters,
                  "roi_sample: null buffer");
    const int64_t slots = std::max<int64_t>(n_cand, 1);
    UMR_CHECK_ARG(workspace && ((uintptr_t)workspace & 3) == 0 && workspace_bytes >= slots * 16,
                  "roi_sample: workspace missing, too small or not 4-byte aligned");
    int32_t* midx = (int32_t*)workspace;
    float* mval = (float*)(midx + slots);
    int32_t* info = (int32_t*)(mval + slots);
    uint32_t* ckey = (uint32_t*)(info + slots);
    hipStream_t s = (hipStream_t)stream;
    if ((phases & 1) && n_chunks > 0) {
        hipLaunchKernelGGL(rs_match_kernel, dim3((unsigned)n_chunks), dim3(RS_THREADS), 0, s, table, n_images, (int)n_cand, iou_threshold,
                           (long long)num_classes, (unsigned)((uint64_t)seed & 0xffffffffu), (unsigned)((uint64_t)seed >> 32), midx, mval,
                           info, ckey);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        hipLaunchKernelGGL(rs_select_kernel, dim3(n_images), dim3(RS_SELECT_THREADS), 0, s, table, (int)n_cand, batch_size, pos_cap, by_key,
                           (long long)num_classes, gt_logit, midx, info, ckey, out_boxes, out_logits, out_classes, out_gt_boxes,
                           out_gt_scores, out_matched_idxs, out_sampled_idxs, counts, counters);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
