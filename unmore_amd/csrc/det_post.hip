// The inference tail of the stage-3 detector (cad/modeling/roi_heads/fast_rcnn.py:52-179, fast_rcnn_inference; roi_heads.py:1048-1091,
// mask_rcnn_inference; meta_arch/rcnn.py:242-256 with Detectron2's detector_postprocess / paste_masks_in_image;
// cad/evaluation/coco_evaluation.py:398-457, instances_to_coco_json): the raw head outputs of a batch -> the kept detections per image
// -> boxes in the original frame -> the pasted masks, as frames (umr_det_paste) or straight as COCO run-length strings
// (umr_det_paste_rle, a third producer for rle_stream.h: the frame is never written).
//
// Selection, three launches for the whole batch over one table (include/umr.h, umr_dp_image), nothing read back, no atomics:
//   dp_candidates_kernel  one workgroup of 256 threads per image.  Walks the (row, class) pairs p = r * K + c in chunks of 256, in
//                         order: a pair is a candidate iff every box and score entry of its row is finite and score[r, c] > score_thresh;
//                         ballots and four wave totals compact the candidates IN ORDER into LDS (score and p, 8 bytes each, at most
//                         8192).  Then every candidate counts its rank, #{j : s_j > s_i or (s_j == s_i and j < i)} -- descending score,
//                         equal scores in candidate order, a permutation because no NaN score is a candidate -- and writes its clipped
//                         box, score and p to that slot of the workspace.
//   dp_mask_kernel        one wave per 64 x 64 tile of an image's upper triangle: the suppression matrix of nms_bitmask.h with the
//                         predicate "same class".
//   dp_scan_kernel        one wave per image: nms_bitmask.h's greedy scan over all ranks, two words per lane (<= 8192), limited to
//                         min(topk, cap).  The kept ranks go through LDS and are written by the whole wave: boxes, scores, classes,
//                         rows, and the count.
// Arithmetic, float32, no contraction, every operation rounded on its own (det_box.h: box_clip; the suppression: nms_bitmask.h):
//   clip        x < 0 ? 0 : (x > width ? width : x)          (a NaN stays a NaN; none arrives here)
//
// The paste (Detectron2's _do_paste_mask: F.grid_sample(align_corners=False, zero padding) of the M x M probabilities, then >= threshold):
// one workgroup of 256 threads per mask; prob = 1 / (1 + expf(-logit)) once into LDS as float32 (bfloat16 logits are widened first).
// Pixel (y, x) of box (x0, y0, x1, y1):
//   gx  = ((x + 0.5) - x0) / (x1 - x0) * 2 - 1                 (the division correctly rounded)
//   ix  = ((gx + 1) * M - 1) * 0.5
//   xl  = floor(ix);  wx1 = ix - xl;  wx0 = (xl + 1) - ix       (taps xl and xl + 1; the same in y with yl, wy0, wy1)
//   nw = wx0 * wy0;  ne = wx1 * wy0;  sw = wx0 * wy1;  se = wx1 * wy1
//   v   = ((nw * p[yl][xl] + ne * p[yl][xl+1]) + sw * p[yl+1][xl]) + se * p[yl+1][xl+1]      (a tap outside [0, M) reads 0)
//   set iff v >= threshold.  xl or yl outside [-1, M - 1] (no tap inside, or a coordinate that is not finite): not set.
// A pixel whose centre lies outside the box in x has ix < -0.5 or ix > M - 0.5, an x-weight below 1/2 and so v < 1/2 <= threshold
// (threshold >= 0.5 is checked by the caller): only the columns [floor(x0), ceil(x1)) and rows [floor(y0), ceil(y1)) inside the frame are
// evaluated.  A box that is not finite or has x1 <= x0 or y1 <= y0 sets nothing.
#pragma clang fp contract(off)
#include "umr_common.h"
#include "det_box.h"
#include "nms_bitmask.h"
#include "rle_stream.h"
#include <algorithm>
#include <float.h>
#include <limits.h>

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_MAX_CAND = 8192;                     // candidates per image: 128 words of removed set = two per lane of the scanning wave
constexpr int DP_MAX_M = 128;                         // M * M float32 probabilities in LDS

static_assert(sizeof(umr_dp_image) == 48 && offsetof(umr_dp_image, mat_first) == 16 && offsetof(umr_dp_image, width) == 44,
              "umr_dp_image is mirrored by _lib.DpImage");

struct DpShape { int K, BC, max_cand, total_cand, total_out; long long total_words; };

__device__ __forceinline__ int dp_words(int n) { return (n + 63) >> 6; }

// what the kernels trust of a table entry before they index with it
__device__ __forceinline__ bool dp_entry_ok(const umr_dp_image& im, const DpShape& sh) {
    if (im.R < 0 || im.R > sh.max_cand / sh.K) return false;
    const int P = im.R * sh.K;
    if (P == 0) return true;
    return im.boxes && im.scores && im.cand_first >= 0 && im.cand_first <= sh.total_cand - P && im.cap >= 0 && im.cap <= P &&
           im.out_first >= 0 && im.out_first <= sh.total_out - im.cap && im.mat_first >= 0 &&
           im.mat_first <= sh.total_words - (long long)P * dp_words(P);
}

struct DpWork { int32_t* n_cand; f32x4* sbox; float* sscore; int32_t* spair; unsigned long long* mat; };

__global__ __launch_bounds__(DP_THREADS) void dp_candidates_kernel(const umr_dp_image* __restrict__ images, DpShape sh, float score_thresh,
                                                                   DpWork ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int wtot[2][4];
    float* s_score = (float*)lds;
    int* s_pair = (int*)(s_score + sh.max_cand);
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const umr_dp_image im = images[k];
    if (!dp_entry_ok(im, sh)) {
        if (tid == 0) ws.n_cand[k] = 0;
        return;
    }
    const int K = sh.K, P = im.R * K, bw = sh.BC * 4;
    int n = 0, par = 0;
    for (int base = 0; base < P; base += DP_THREADS) {
        const int p = base + tid;
        bool cand = false;
        float sc = 0.f;
        if (p < P) {
            const int r = p / K, c = p - r * K;
            const float* b = im.boxes + (int64_t)r * bw;
            const float* s = im.scores + (int64_t)r * (K + 1);
            bool ok = true;
            for (int q = 0; q < bw; ++q) ok = ok && box_finite(b[q]);
            for (int q = 0; q <= K; ++q) ok = ok && box_finite(s[q]);
            sc = s[c];
            cand = ok && sc > score_thresh;
        }
        const unsigned long long vote = __ballot(cand);
        if (lane == 0) wtot[par][wv] = __popcll(vote);
        __syncthreads();
        int off = n + __popcll(vote & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; ++w) off += wtot[par][w];
        if (cand && off < sh.max_cand) {                            // off < P <= max_cand always
            s_score[off] = sc;
            s_pair[off] = p;
        }
        n += wtot[par][0] + wtot[par][1] + wtot[par][2] + wtot[par][3];
        par ^= 1;
    }
    __syncthreads();
    if (tid == 0) ws.n_cand[k] = n;
    // the rank count stands here and in rpn.hip's rpn_rank_kernel (on keys): moved into one inline function of det_box.h, this
    // kernel compiled to other code (same registers, another schedule) that measured about 1 % slower on the MI355X
    const int n4 = n & ~3;
    for (int i = tid; i < n; i += DP_THREADS) {
        const float si = s_score[i];
        int rank = 0;
        for (int j = 0; j < n4; j += 4) {
            const f32x4 v = *(const f32x4*)(s_score + j);
            rank += (v[0] > si || (v[0] == si && j < i)) + (v[1] > si || (v[1] == si && j + 1 < i)) +
                    (v[2] > si || (v[2] == si && j + 2 < i)) + (v[3] > si || (v[3] == si && j + 3 < i));
        }
        for (int j = n4; j < n; ++j) {
            const float sj = s_score[j];
            rank += (sj > si || (sj == si && j < i));
        }
        const int p = s_pair[i], r = p / K, c = p - r * K;
        const float* b = im.boxes + (int64_t)r * bw + (sh.BC == 1 ? 0 : c * 4);
        const f32x4 box = {box_clip(b[0], im.width), box_clip(b[1], im.height), box_clip(b[2], im.width), box_clip(b[3], im.height)};
        if (rank < n) {                                             // a permutation of [0, n): always
            const int64_t at = (int64_t)im.cand_first + rank;
            ws.sbox[at] = box;
            ws.sscore[at] = si;
            ws.spair[at] = p;
        }
    }
}

__global__ __launch_bounds__(64) void dp_mask_kernel(const umr_dp_image* __restrict__ images, DpShape sh, float nms_thresh, DpWork ws) {
    __shared__ f32x4 cbox[64];
    __shared__ int ccls[64];
    const int k = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x, t = threadIdx.x;
    const umr_dp_image im = images[k];
    if (!dp_entry_ok(im, sh)) return;
    const int P = im.R * sh.K, words = dp_words(P);
    const int n = min(ws.n_cand[k], P);
    if (cb < rb || rb * 64 >= n || cb * 64 >= n) return;            // the upper triangle of the ranks that exist
    const int64_t cf = im.cand_first;
    const int j0 = cb * 64, nj = min(64, n - j0);
    if (t < nj) {
        cbox[t] = ws.sbox[cf + j0 + t];
        ccls[t] = ws.spair[cf + j0 + t] % sh.K;
    }
    __syncthreads();
    const int i = rb * 64 + t;
    if (i >= n) return;
    const int cls = ws.spair[cf + i] % sh.K;
    ws.mat[im.mat_first + (int64_t)i * words + cb] =
        nms_tile_word(ws.sbox[cf + i], i, cbox, j0, nj, nms_thresh, [&](int jj) { return ccls[jj] == cls; });
}

__global__ __launch_bounds__(64) void dp_scan_kernel(const umr_dp_image* __restrict__ images, DpShape sh, int topk, DpWork ws,
                                                     float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                     int64_t* __restrict__ out_classes, int64_t* __restrict__ out_rows,
                                                     int32_t* __restrict__ counts) {
    __shared__ int kept_rank[DP_MAX_CAND];
    const int k = blockIdx.x, lane = threadIdx.x;
    const umr_dp_image im = images[k];
    if (!dp_entry_ok(im, sh)) {
        if (lane == 0) counts[k] = 0;
        return;
    }
    const int P = im.R * sh.K, words = dp_words(P);
    const int n = min(ws.n_cand[k], P), nw = dp_words(n);
    const int limit = topk >= 0 ? min(topk, im.cap) : im.cap;
    const unsigned long long* mat = ws.mat + im.mat_first;
    // the row pitch comes from P, the words that dp_mask_kernel wrote from n
    const unsigned long long valid[2] = {nms_all_valid(lane, n), nms_all_valid(lane + 64, n)};
    const int kept = nms_greedy_scan<2>(mat, words, nw, n, valid, limit, kept_rank);
    __syncthreads();
    if (lane == 0) counts[k] = kept;
    for (int j = lane; j < kept; j += 64) {
        const int64_t src = (int64_t)im.cand_first + kept_rank[j], dst = (int64_t)im.out_first + j;
        const f32x4 b = ws.sbox[src];
        const int p = ws.spair[src];
        *(f32x4*)(out_boxes + dst * 4) = b;
        out_scores[dst] = ws.sscore[src];
        out_classes[dst] = p % sh.K;
        out_rows[dst] = p / sh.K;
    }
}

// ---------------------------------------------------------------------------------------------------------------- to the original frame
// Boxes.scale by (sx, sy), Boxes.clip to (H, W), nonempty: rec [n, 8] = x0, y0, x1, y1, x1 - x0, y1 - y0, kept (1 / 0), 0
__global__ __launch_bounds__(DP_THREADS) void dp_scale_kernel(const float* __restrict__ boxes, const float* __restrict__ rowinfo, int n,
                                                              float* __restrict__ rec) {
    const int i = blockIdx.x * DP_THREADS + threadIdx.x;
    if (i >= n) return;
    const float sx = rowinfo[i * 4], sy = rowinfo[i * 4 + 1];
    const float H = (float)((const int32_t*)rowinfo)[i * 4 + 2], W = (float)((const int32_t*)rowinfo)[i * 4 + 3];
    const float x0 = box_clip(boxes[i * 4] * sx, W), y0 = box_clip(boxes[i * 4 + 1] * sy, H);
    const float x1 = box_clip(boxes[i * 4 + 2] * sx, W), y1 = box_clip(boxes[i * 4 + 3] * sy, H);
    const float w = x1 - x0, h = y1 - y0;
    float* o = rec + (int64_t)i * 8;
    o[0] = x0; o[1] = y0; o[2] = x1; o[3] = y1; o[4] = w; o[5] = h;
    o[6] = (w > 0.f && h > 0.f) ? 1.f : 0.f;
    o[7] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- the paste
struct DpPaste {
    const float* prob;                // [M, M] in LDS
    int M;
    float x0, y0, x1, y1, thr;
    int vx, vy, vw, vh;               // the evaluated columns and rows: the box rounded outward, inside the frame
    __device__ __forceinline__ int bit(int x, int y) const {
        const float fM = (float)M;
        const float gx = __fdiv_rn(((float)x + 0.5f) - x0, x1 - x0) * 2.f - 1.f;
        const float gy = __fdiv_rn(((float)y + 0.5f) - y0, y1 - y0) * 2.f - 1.f;
        const float ix = ((gx + 1.f) * fM - 1.f) * 0.5f, iy = ((gy + 1.f) * fM - 1.f) * 0.5f;
        const float xl = floorf(ix), yl = floorf(iy);
        if (!(xl >= -1.f && xl <= fM - 1.f && yl >= -1.f && yl <= fM - 1.f)) return 0;
        const float wx1 = ix - xl, wx0 = (xl + 1.f) - ix, wy1 = iy - yl, wy0 = (yl + 1.f) - iy;
        const int xi = (int)xl, yi = (int)yl;
        const bool xa = xi >= 0, xb = xi + 1 < M, ya = yi >= 0, yb = yi + 1 < M;
        const float v_nw = (xa && ya) ? prob[yi * M + xi] : 0.f, v_ne = (xb && ya) ? prob[yi * M + xi + 1] : 0.f;
        const float v_sw = (xa && yb) ? prob[(yi + 1) * M + xi] : 0.f, v_se = (xb && yb) ? prob[(yi + 1) * M + xi + 1] : 0.f;
        const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
        const float v = ((nw * v_nw + ne * v_ne) + sw * v_sw) + se * v_se;
        return v >= thr ? 1 : 0;
    }
};

// fills the LDS probabilities of mask k and its evaluated rectangle; false: nothing is set
__device__ __forceinline__ bool dp_paste_setup(const void* __restrict__ logits, int dtype, int C, int M, const int64_t* __restrict__ classes,
                                               const float* __restrict__ box, float thr, int H, int W, int k, float* prob, DpPaste& ps) {
    const int MM = M * M;
    long long ch = 0;
    if (C > 1) {
        ch = classes[k];
        if (ch < 0 || ch >= C) ch = -1;                             // a class without a channel: an empty mask
    }
    const int64_t at = ((int64_t)k * C + (ch < 0 ? 0 : ch)) * MM;
    for (int i = threadIdx.x; i < MM; i += blockDim.x) {
        const float v = dtype == UMR_BF16 ? (float)((const bf16_t*)logits)[at + i] : ((const float*)logits)[at + i];
        prob[i] = __fdiv_rn(1.f, 1.f + expf(-v));
    }
    const float x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    ps = DpPaste{prob, M, x0, y0, x1, y1, thr, 0, 0, 0, 0};
    if (ch < 0 || !(box_finite(x0) && box_finite(y0) && box_finite(x1) && box_finite(y1)) || !(x1 > x0 && y1 > y0)) return false;
    const float fW = (float)W, fH = (float)H;
    const int xs = (int)floorf(box_clip(x0, fW)), xe = (int)ceilf(box_clip(x1, fW));
    const int ys = (int)floorf(box_clip(y0, fH)), ye = (int)ceilf(box_clip(y1, fH));
    ps.vx = xs; ps.vy = ys; ps.vw = xe - xs; ps.vh = ye - ys;
    return ps.vw > 0 && ps.vh > 0;
}

__global__ __launch_bounds__(DP_THREADS) void dp_paste_kernel(const void* __restrict__ logits, int dtype, int C, int M,
                                                              const int64_t* __restrict__ classes, const float* __restrict__ boxes,
                                                              int box_stride, float thr, int H, int W, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int k = blockIdx.x;
    DpPaste ps;
    const bool any = dp_paste_setup(logits, dtype, C, M, classes, boxes + (int64_t)k * box_stride, thr, H, W, k, (float*)lds, ps);
    __syncthreads();
    if (!any) return;
    uint8_t* o = out + (int64_t)k * H * W;
    const int total = ps.vw * ps.vh;                                // <= H * W < 2^31
    for (int i = threadIdx.x; i < total; i += DP_THREADS) {
        const int yy = i / ps.vw, xx = i - yy * ps.vw;
        const int x = ps.vx + xx, y = ps.vy + yy;
        o[(int64_t)y * W + x] = (uint8_t)ps.bit(x, y);              // the frame arrives zeroed
    }
}

// The stream of rle.hip's PasteProducer over the evaluated rectangle: its columns top to bottom; when the rectangle is lower than the
// frame every column gets one more position below its last row (value 0), so that a pixel's predecessor in the stream has the value of
// its predecessor in the frame's column-major order; a rectangle as high as the frame has no such position between its columns and gets
// one after its last column when that is not the frame's last.
struct DpProducer {
    DpPaste ps;
    uint32_t H, hl;                   // hl = vh + (vh < H): positions per column
    __device__ __forceinline__ int value(uint32_t p) const {
        const uint32_t cx = p / hl, cy = p - cx * hl;
        if ((int)cy >= ps.vh || (int)cx >= ps.vw) return 0;
        return ps.bit(ps.vx + (int)cx, ps.vy + (int)cy);
    }
    __device__ __forceinline__ int before() const { return 0; }
    __device__ __forceinline__ uint32_t gpos(uint32_t p) const {
        const uint32_t cx = p / hl, cy = p - cx * hl;
        return ((uint32_t)ps.vx + cx) * H + (uint32_t)ps.vy + cy;
    }
};

template <bool WRITE>
__global__ __launch_bounds__(RLE_THREADS) void dp_paste_rle_kernel(const void* __restrict__ logits, int dtype, int C, int M,
                                                                   const int64_t* __restrict__ classes, const float* __restrict__ boxes,
                                                                   int box_stride, const int32_t* __restrict__ frames, int frame_stride,
                                                                   float thr, int64_t* __restrict__ sizes, const int64_t* __restrict__ offsets,
                                                                   uint8_t* __restrict__ chars, int64_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ RleShared sh;
    const int k = blockIdx.x;
    int H = frames[(int64_t)k * frame_stride], W = frames[(int64_t)k * frame_stride + 1];
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) H = W = 0;       // checked by the caller: an empty record of size 0
    DpPaste ps;
    const bool any = dp_paste_setup(logits, dtype, C, M, classes, boxes + (int64_t)k * box_stride, thr, H, W, k, (float*)lds, ps);
    __syncthreads();
    RleState st;
    const int64_t ob = WRITE ? offsets[k] : 0;
    if (any) {
        const uint32_t hl = (uint32_t)ps.vh + (ps.vh < H ? 1u : 0u);
        const DpProducer prod{ps, (uint32_t)H, hl};
        uint32_t n = hl * (uint32_t)ps.vw;
        if (ps.vh == H && ps.vx + ps.vw < W) ++n;                               // the first zero right of a rectangle as high as the frame
        if (ps.vh < H && ps.vy + ps.vh == H && ps.vx + ps.vw == W) --n;         // the position below the frame's last pixel is the end
        rle_stream<WRITE>(prod, n, sh, st, chars, ob, cap);
    }
    rle_finish<WRITE>(st, (uint32_t)H * (uint32_t)W, k, sizes, chars, ob, cap);
}

int dp_check_paste(const void* logits, int dtype, int64_t N, int C, int M, const int64_t* classes, const float* boxes, int box_stride,
                   float threshold) {
    UMR_CHECK_ARG(logits && boxes && N > 0 && N <= INT_MAX && C > 0 && M > 0, "det_paste: bad arguments");
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "det_paste: logits must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(C == 1 || classes, "det_paste: class-specific logits need the classes");
    UMR_CHECK_ARG(box_stride >= 4, "det_paste: a box has four coordinates");
    UMR_CHECK_ARG(threshold >= 0.5f && threshold <= 1.f, "det_paste: the threshold must lie in [0.5, 1]");
    if (M > DP_MAX_M) return umr_set_error(UMR_ERR_UNSUPPORTED, "det_paste: M * M probabilities must fit 64 KiB of LDS (M <= 128)");
    return UMR_OK;
}

}  // namespace

extern "C" int64_t umr_det_select_workspace(int n_images, int64_t total_cand, int64_t total_words) {
    if (n_images < 0 || total_cand < 0 || total_words < 0 || total_cand > INT_MAX) return -1;
    const int64_t nc = ((int64_t)std::max(n_images, 1) * 4 + 15) & ~(int64_t)15;
    const int64_t c = std::max<int64_t>(total_cand, 1);
    return nc + c * 16 + ((c * 4 + 15) & ~(int64_t)15) * 2 + std::max<int64_t>(total_words, 1) * 8;
}

extern "C" int umr_det_select(const umr_dp_image* images, int n_images, int K, int box_classes, int64_t total_cand, int max_cand,
                              int64_t total_words, int64_t total_out, float score_thresh, float nms_thresh, int topk, int phases,
                              float* out_boxes, float* out_scores, int64_t* out_classes, int64_t* out_rows, int32_t* counts, void* workspace,
                              int64_t workspace_bytes, umr_stream_t stream) {
    UMR_CHECK_ARG(images && n_images > 0 && n_images <= 65535, "det_select: between 1 and 65535 images");
    UMR_CHECK_ARG(K > 0 && (box_classes == 1 || box_classes == K), "det_select: K classes, and boxes for one class or for K");
    UMR_CHECK_ARG(max_cand >= 0 && total_cand >= 0 && total_cand <= INT_MAX && total_words >= 0 && total_out >= 0 && total_out <= total_cand,
                  "det_select: negative extent");
    if (max_cand > DP_MAX_CAND) return umr_set_error(UMR_ERR_UNSUPPORTED, "det_select: at most 8192 (row, class) pairs per image");
    UMR_CHECK_ARG(score_thresh == score_thresh && nms_thresh == nms_thresh, "det_select: a threshold is NaN");
    UMR_CHECK_ARG(counts && workspace && ((uintptr_t)workspace & 15) == 0, "det_select: null or misaligned buffer");
    UMR_CHECK_ARG(total_out == 0 || (out_boxes && out_scores && out_classes && out_rows), "det_select: null output");
    UMR_CHECK_ARG(((uintptr_t)out_boxes & 15) == 0, "det_select: out_boxes not 16-byte aligned");
    UMR_CHECK_ARG(workspace_bytes >= umr_det_select_workspace(n_images, total_cand, total_words), "det_select: workspace too small");
    const int64_t c = std::max<int64_t>(total_cand, 1);
    unsigned char* base = (unsigned char*)workspace;
    DpWork ws;
    ws.n_cand = (int32_t*)base;
    base += ((int64_t)n_images * 4 + 15) & ~(int64_t)15;
    ws.sbox = (f32x4*)base;
    base += c * 16;
    ws.sscore = (float*)base;
    base += (c * 4 + 15) & ~(int64_t)15;
    ws.spair = (int32_t*)base;
    base += (c * 4 + 15) & ~(int64_t)15;
    ws.mat = (unsigned long long*)base;
    const DpShape sh{K, box_classes, max_cand, (int)total_cand, (int)total_out, (long long)total_words};
    hipStream_t s = (hipStream_t)stream;
    if (phases & 1) {
        const size_t lds = (size_t)std::max(max_cand, 4) * 8;
        UMR_SET_MAX_LDS_ONCE(dp_candidates_kernel, DP_MAX_CAND * 8);
        hipLaunchKernelGGL(dp_candidates_kernel, dim3(n_images), dim3(DP_THREADS), lds, s, images, sh, score_thresh, ws);
        UMR_LAUNCH_CHECK();
    }
    const int tiles = (max_cand + 63) / 64;
    if ((phases & 2) && tiles > 0) {
        hipLaunchKernelGGL(dp_mask_kernel, dim3(tiles, tiles, n_images), dim3(64), 0, s, images, sh, nms_thresh, ws);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 4) {
        hipLaunchKernelGGL(dp_scan_kernel, dim3(n_images), dim3(64), 0, s, images, sh, topk, ws, out_boxes, out_scores, out_classes, out_rows,
                           counts);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}

extern "C" int umr_det_scale(const float* boxes, const void* rowinfo, int64_t n, float* rec, umr_stream_t stream) {
    UMR_CHECK_ARG(boxes && rowinfo && rec && n > 0 && n <= INT_MAX / 8, "det_scale: bad arguments");
    hipLaunchKernelGGL(dp_scale_kernel, dim3((int)((n + DP_THREADS - 1) / DP_THREADS)), dim3(DP_THREADS), 0, (hipStream_t)stream, boxes,
                       (const float*)rowinfo, (int)n, rec);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_det_paste(const void* logits, int dtype, int64_t N, int C, int M, const int64_t* classes, const float* boxes,
                             int box_stride, int H, int W, float threshold, uint8_t* out, umr_stream_t stream) {
    if (int st = dp_check_paste(logits, dtype, N, C, M, classes, boxes, box_stride, threshold)) return st;
    UMR_CHECK_ARG(out && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "det_paste: a frame with 0 < H * W < 2^31 and its buffer");
    UMR_SET_MAX_LDS_ONCE(dp_paste_kernel, DP_MAX_M * DP_MAX_M * 4);
    hipLaunchKernelGGL(dp_paste_kernel, dim3((int)N), dim3(DP_THREADS), (size_t)M * M * 4, (hipStream_t)stream, logits, dtype, C, M, classes, boxes,
                       box_stride, threshold, H, W, out);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_det_paste_rle(const void* logits, int dtype, int64_t N, int C, int M, const int64_t* classes, const float* boxes,
                                 int box_stride, const int32_t* frames, int frame_stride, float threshold, int64_t* sizes,
                                 const int64_t* offsets, uint8_t* chars, int64_t chars_capacity, umr_stream_t stream) {
    if (int st = dp_check_paste(logits, dtype, N, C, M, classes, boxes, box_stride, threshold)) return st;
    UMR_CHECK_ARG(frames && frame_stride >= 2, "det_paste_rle: one (H, W) per mask");
    UMR_CHECK_ARG(rle_buffers_ok(sizes, offsets, chars, chars_capacity),
                  "det_paste_rle: the measure pass needs sizes; the write pass needs offsets, chars and a positive chars_capacity");
    const size_t lds = (size_t)M * M * 4;
    hipStream_t s = (hipStream_t)stream;
    if (chars) {
        UMR_SET_MAX_LDS_ONCE(dp_paste_rle_kernel<true>, DP_MAX_M * DP_MAX_M * 4);
        hipLaunchKernelGGL(dp_paste_rle_kernel<true>, dim3((int)N), dim3(RLE_THREADS), lds, s, logits, dtype, C, M, classes, boxes, box_stride,
                           frames, frame_stride, threshold, sizes, offsets, chars, chars_capacity);
    } else {
        UMR_SET_MAX_LDS_ONCE(dp_paste_rle_kernel<false>, DP_MAX_M * DP_MAX_M * 4);
        hipLaunchKernelGGL(dp_paste_rle_kernel<false>, dim3((int)N), dim3(RLE_THREADS), lds, s, logits, dtype, C, M, classes, boxes, box_stride,
                           frames, frame_stride, threshold, sizes, offsets, chars, chars_capacity);
    }
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
