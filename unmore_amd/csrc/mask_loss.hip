// Mask-head targets and the score-weighted mask loss of the stage-3 detector (cad/modeling/roi_heads/roi_heads.py:963-1045,
// mask_rcnn_loss_weighted; the crop is Detectron2's BitMasks.crop_and_resize = ROIAlign((M, M), 1.0, sampling_ratio=0, aligned=True) of
// the float mask, then >= 0.5).  One workgroup of 256 threads per proposal (several for a large one), a finishing launch of one
// workgroup; no atomics, no flags between workgroups, every sum in a fixed order: the same input gives the same bytes on every run.
//
//   ml_main_kernel    finds its proposal's image in the table (include/umr.h, umr_ml_image), checks what lives on the device (mask
//                     index, box), and lays the proposal's sample rows and columns into LDS once: per bin the run of sample indices whose
//                     coordinate falls inside [-1, H] (or [-1, W]), each as (low index, fraction), -1 = outside.  A thread owns the bins
//                     tid, tid + 256, ... of its workgroup's rows of bins: it walks the bin's samples rows-outer / columns-inner as the reference does, reads the four taps
//                     from the byte mask, thresholds the average, and takes the BCE term, the gradient element and the counters from the
//                     one logit it loads for that bin.  A fixed butterfly and a fixed sum over the four waves make one partial per
//                     workgroup: the weighted loss as double and five int32 counts.
//                     The grid is R x S, S = ceil(M * M / 256).  A proposal's samples grow with its area and one workgroup walks them
//                     alone (measured: the largest of 2048 proposals took 46 % of the whole launch by itself), so a proposal of more
//                     than 65536 samples -- by the bound below, known before any table is built -- is shared by the S workgroups of
//                     its grid row, ceil(M / S) rows of bins each (M = 28: 4 x 7 rows, one pass of bins per workgroup instead of
//                     four); for a smaller one the workgroups (r, 1 ..) write an empty partial and leave.  A bin is always one
//                     thread's, so its sum is the same either way.
//   ml_finish_kernel  sums the R * S partials, thread t the partials t, t + 256, ... in index order, then the same tree:
//                     loss / (R * M * M) as float32, the five counters as int64.
//
// Arithmetic of a target, float32, no contraction, every operation rounded on its own (torchvision's roi_align, aligned=True):
//   start = x1 - .5f;  roi = (x2 - .5f) - start;  bin = roi / M;  grid = (int)ceilf(roi / M);  count = max(grid_h * grid_w, 1)
//   coordinate(p, i) = start + p * bin + (i + .5f) * bin / grid          [= (start + (p * bin)) + (((i + .5f) * bin) / grid)]
//   outside [-1, size]: the sample adds 0.  Else c <= 0 -> 0; low = (int)c; low >= size - 1 -> low = high = size - 1, c = low; else
//   high = low + 1; l = c - low, h = 1 - l;  sample = hy*hx*v1 + hy*lx*v2 + ly*hx*v3 + ly*lx*v4 (v = 0 / 1: a product is its weight or 0);
//   target = (sum over iy outer, ix inner) / count >= .5f.  roi <= 0 on either axis: no samples, an all-zero target.
//
// What bounds the work.  coordinate(p, i) is a chain of monotone roundings, so it does not decrease with i, and the indices of a bin
// that fall inside [-1, size] are one run [a, b): both ends are found by bisection ON THE FLOAT32 EXPRESSION ITSELF (at most 22 steps;
// a box coordinate is at most 2^20 in magnitude, so grid <= 2^21 / M + 1).  The samples outside the run fail the per-sample test,
// which stays, and add exactly 0: the sum is the reference's.  Inside one bin the samples are bin / grid = roi / (M * ceil(roi / M))
// apart, more than 1/2 whenever grid >= 2, and the bins do not overlap; float32 moves a coordinate by less than 1 (the terms are below
// 2^21).  So all bins of an axis together hold at most 2 * (size + 4) + M samples inside [-1, size]:
//   work per proposal <= (2 * (H + 4) + M) * (2 * (W + 4) + M) samples of four taps, whatever the box,
// and that is also the LDS the tables take (8 bytes per sample row and column).  A proposal whose runs would not fit -- which the bound
// rules out -- is treated as a bad one rather than written past the tables.
//
// Bad proposals: mask index outside [0, G), a box coordinate that is not finite or beyond +-2^20, a table entry that contradicts
// itself.  They get an empty target (the loss then runs against it) and are counted in the fifth counter.  A class outside [0, C)
// (C > 1) is counted there too; it adds no loss, no count and a zero gradient, since no channel is its own.
#pragma clang fp contract(off)
#include "umr_common.h"
#include "roi_align_axis.h"
#include <algorithm>

namespace {

constexpr int ML_THREADS = 256;
constexpr int ML_MAX_SIDE = 512;
constexpr float ML_MAX_COORD = 1048576.f;            // 2^20
constexpr int64_t ML_MAX_LDS = 160 * 1024;
constexpr long long ML_SPLIT_SAMPLES = 65536;        // a proposal with more samples than this is shared by the workgroups of its grid row

static_assert(sizeof(umr_ml_image) == 48 && offsetof(umr_ml_image, index64) == 44, "umr_ml_image is mirrored by _lib.MlImage");

using Partial = SumPartial<1, 5>;                    // one per workgroup, 32 bytes: the weighted loss; incorrect, positive, false positive,
                                                     // false negative, bad

__host__ __device__ inline int ml_cap(int size, int M) { return 2 * (size + 4) + M; }
inline int ml_slices(int M) { return (M * M + ML_THREADS - 1) / ML_THREADS; }      // workgroups per proposal: one pass of bins each when all are used
__host__ __device__ inline int64_t ml_lds_bytes(int M, int max_h, int max_w) {
    // 192 bytes of reduction scratch, 4 * M + 2 ints of runs, then the sample rows and columns
    return 200 + 16 * (int64_t)M + 8 * ((int64_t)ml_cap(max_h, M) + ml_cap(max_w, M));
}

template <typename T, bool LOSS>
__global__ __launch_bounds__(ML_THREADS) void ml_main_kernel(const umr_ml_image* __restrict__ images, int n_images, int R, int C, int M,
                                                             int max_h, int max_w, const T* __restrict__ logits,
                                                             const int64_t* __restrict__ classes, const float* __restrict__ weights,
                                                             float inv_n, uint8_t* __restrict__ targets, T* __restrict__ grad,
                                                             Partial* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ml_smem[];
    double* red_d = (double*)ml_smem;                                  // [4]
    long long* red_n = (long long*)(ml_smem + 32);                     // [4][5]
    int* lo_run = (int*)(ml_smem + 192);                               // [2][M]: first sample index of the run of bin p, rows then columns
    int* off_run = lo_run + 2 * M;                                     // [2][M + 1]: where the run of bin p starts in its table
    const int cap_h = ml_cap(max_h, M), cap_w = ml_cap(max_w, M);
    int2* ent = (int2*)(ml_smem + 200 + 16 * M);                       // [cap_h] sample rows, then [cap_w] sample columns
    const int tid = threadIdx.x, r = blockIdx.x;
    const int MM = M * M;

    // ---- the proposal's image: the last table entry whose first proposal is <= r (entries without proposals share a `first`)
    int lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (images[mid].first <= r) lo = mid; else hi = mid;
    }
    const umr_ml_image im = images[lo];
    const int j = r - im.first, H = im.H, W = im.W;
    bool ok = im.masks && im.boxes && H > 0 && W > 0 && H <= max_h && W <= max_w && im.G >= 0 && j >= 0 && j < im.R;
    long long g = -1;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (ok) {
        g = !im.index ? (long long)j : im.index64 ? ((const long long*)im.index)[j] : (long long)((const int32_t*)im.index)[j];
        const float* b = im.boxes + (int64_t)j * 4;
        x1 = b[0]; y1 = b[1]; x2 = b[2]; y2 = b[3];
    }
    ok = ok && g >= 0 && g < im.G;
    ok = ok && fabsf(x1) <= ML_MAX_COORD && fabsf(y1) <= ML_MAX_COORD && fabsf(x2) <= ML_MAX_COORD && fabsf(y2) <= ML_MAX_COORD;   // NaN fails
    int ch = 0;
    bool class_ok = true;
    if (LOSS && C > 1) {
        const long long c = classes[r];
        class_ok = c >= 0 && c < C;
        ch = class_ok ? (int)c : 0;
    }

    // ---- geometry
    const float start_w = x1 - .5f, start_h = y1 - .5f;
    const float roi_w = (x2 - .5f) - start_w, roi_h = (y2 - .5f) - start_h;
    const float bin_w = __fdiv_rn(roi_w, (float)M), bin_h = __fdiv_rn(roi_h, (float)M);
    bool sampled = ok && roi_w > 0.f && roi_h > 0.f;
    const int grid_w = sampled ? (int)ceilf(bin_w) : 0, grid_h = sampled ? (int)ceilf(bin_h) : 0;
    sampled = sampled && grid_w > 0 && grid_h > 0;                      // a denormal roi: bin rounds to 0, the reference's loops are empty too
    const float count = fmaxf((float)((long long)grid_h * grid_w), 1.f);

    // ---- the workgroups (r, 0 .. gridDim.y - 1) share a large proposal by whole rows of bins; a small one is workgroup (r, 0)'s alone
    const long long est = !sampled ? 0 : min((long long)grid_h * M, (long long)cap_h) * min((long long)grid_w * M, (long long)cap_w);
    const int slices = est > ML_SPLIT_SAMPLES ? (int)gridDim.y : 1;
    const int rows_per = (M + slices - 1) / slices;
    const int ph0 = min((int)blockIdx.y * rows_per, M), ph1 = (int)blockIdx.y < slices ? min(ph0 + rows_per, M) : ph0;
    Partial* partial = LOSS ? partials + ((int64_t)r * gridDim.y + blockIdx.y) : nullptr;
    if (ph0 >= ph1) {                                                   // workgroup-uniform: nothing of this proposal is left for this workgroup
        if (LOSS && tid == 0) *partial = Partial{};
        return;
    }

    // ---- the runs of samples inside the frame, per bin and axis (axis 0: rows against H, axis 1: columns against W)
    if (sampled) {
        for (int k = tid; k < 2 * M; k += ML_THREADS) {
            const int axis = k >= M, p = k - axis * M;
            const float start = axis ? start_w : start_h, bin = axis ? bin_w : bin_h;
            const int grid = axis ? grid_w : grid_h, size = axis ? W : H;
            const int a = roi_axis_first(start, bin, grid, p, -1.f, false);
            const int b = max(a, roi_axis_first(start, bin, grid, p, (float)size, true));
            lo_run[k] = a;
            off_run[axis * (M + 1) + p + 1] = b - a;
        }
        __syncthreads();
        if (tid == 0 || tid == 64) {                                    // two waves, one axis each: M <= 512 short adds
            int* off = off_run + (tid ? M + 1 : 0);
            off[0] = 0;
            for (int p = 0; p < M; ++p) off[p + 1] += off[p];
        }
        __syncthreads();
        if (off_run[M] > cap_h || off_run[2 * M + 1] > cap_w) {          // ruled out by the bound at the head of the file; never write past
            sampled = false;
            ok = false;
        }
    }
    const int* off_h = off_run;
    const int* off_w = off_run + M + 1;
    int2* ent_h = ent;
    int2* ent_w = ent + cap_h;
    if (sampled) {                                                      // workgroup-uniform
        for (int p = 0; p < M; ++p) {
            for (int k = tid; p >= ph0 && p < ph1 && k < off_h[p + 1] - off_h[p]; k += ML_THREADS)
                ent_h[off_h[p] + k] = roi_axis_entry(roi_axis_coord(start_h, bin_h, grid_h, p, lo_run[p] + k), H);
            for (int k = tid; k < off_w[p + 1] - off_w[p]; k += ML_THREADS)
                ent_w[off_w[p] + k] = roi_axis_entry(roi_axis_coord(start_w, bin_w, grid_w, p, lo_run[M + p] + k), W);
        }
        __syncthreads();
    }

    // ---- bins
    const uint8_t* m = sampled ? im.masks + (int64_t)g * H * W : nullptr;
    const float w = (LOSS && weights) ? weights[r] : 1.f;
    double lsum[1] = {0.0};
    long long n[5] = {0, 0, 0, 0, 0};
    for (int bin = ph0 * M + tid; bin < ph1 * M; bin += ML_THREADS) {
        const int ph = bin / M, pw = bin - ph * M;
        float acc = 0.f;
        if (sampled) {
            const int b0 = off_w[pw], b1 = off_w[pw + 1];
            for (int a = off_h[ph]; a < off_h[ph + 1]; ++a) {
                const int2 ey = ent_h[a];
                if (ey.x < 0) continue;
                const float ly = __int_as_float(ey.y), hy = 1.f - ly;
                const uint8_t* row0 = m + (int64_t)ey.x * W;
                const uint8_t* row1 = row0 + (ey.x < H - 1 ? W : 0);
                for (int b = b0; b < b1; ++b) {
                    const int2 ex = ent_w[b];
                    if (ex.x < 0) continue;
                    const float lx = __int_as_float(ex.y), hx = 1.f - lx;
                    const int xh = ex.x + (ex.x < W - 1 ? 1 : 0);
                    const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                    const float val = (row0[ex.x] ? w1 : 0.f) + (row0[xh] ? w2 : 0.f) + (row1[ex.x] ? w3 : 0.f) + (row1[xh] ? w4 : 0.f);
                    acc += val;
                }
            }
        }
        const bool t = __fdiv_rn(acc, count) >= .5f;
        if (targets) targets[(int64_t)r * MM + bin] = t ? 1 : 0;
        if constexpr (LOSS) {
            float gv = 0.f;
            if (class_ok) {
                const float x = to_f32<T>(logits[((int64_t)r * C + ch) * MM + bin]);
                const float e = expf(-fabsf(x));
                const float bce = (t ? 0.f : x) + fmaxf(-x, 0.f) + log1pf(e);
                lsum[0] += (double)(w * bce);
                const bool wrong = (x > 0.f) != t;
                n[0] += wrong; n[1] += t; n[2] += wrong && !t; n[3] += wrong && t;
                const float pp = 1.f / (1.f + e), qq = e * pp;          // sigmoid(|x|), sigmoid(-|x|)
                const float d = t ? -(x >= 0.f ? qq : pp) : (x >= 0.f ? pp : qq);   // sigmoid(x) - t without the cancellation
                gv = (w * d) * inv_n;
            }
            for (int c = 0; c < C; ++c) grad[((int64_t)r * C + c) * MM + bin] = from_f32<T>(c == ch ? gv : 0.f);
        }
    }
    if constexpr (LOSS) {
        block_sum_fixed(lsum, n, red_d, red_n);
        if (tid == 0) {
            Partial q;
            q.d[0] = lsum[0];
            q.c[0] = (int32_t)n[0]; q.c[1] = (int32_t)n[1]; q.c[2] = (int32_t)n[2]; q.c[3] = (int32_t)n[3];
            q.c[4] = (blockIdx.y == 0 && !(ok && class_ok)) ? 1 : 0;
            q.c[5] = 0;
            *partial = q;
        }
    }
}

__global__ __launch_bounds__(ML_THREADS) void ml_finish_kernel(const Partial* __restrict__ partials, int64_t n_partials, double n_elements,
                                                               float* __restrict__ loss, int64_t* __restrict__ counts) {
    __shared__ double red_d[4];
    __shared__ long long red_n[20];
    double d[1];
    long long n[5];
    partials_sum_fixed(partials, n_partials, d, n, red_d, red_n);
    if (threadIdx.x == 0) {
        loss[0] = n_partials > 0 ? (float)(d[0] / n_elements) : 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k) counts[k] = n[k];
    }
}

int ml_check_common(const umr_ml_image* images, int n_images, int64_t R, int M, int max_h, int max_w) {
    UMR_CHECK_ARG(n_images >= 0 && R >= 0 && max_h >= 0 && max_w >= 0, "mask_loss: negative extent");
    UMR_CHECK_ARG(R <= INT_MAX, "mask_loss: more than 2^31 - 1 proposals");
    UMR_CHECK_ARG(M >= 1 && M <= ML_MAX_SIDE, "mask_loss: the side must be in [1, 512]");
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(images && n_images > 0, "mask_loss: proposals without an image table");
    UMR_CHECK_ARG(max_h >= 1 && max_w >= 1, "mask_loss: max_h / max_w must be the largest frame in the table");
    UMR_CHECK_ARG((int64_t)max_h + max_w < (1 << 20) && ml_lds_bytes(M, max_h, max_w) <= ML_MAX_LDS,
                  "mask_loss: the sample tables of a frame this large do not fit the LDS (16 * (H + W) + 32 * M + 328 bytes <= 160 KiB)");
    return UMR_OK;
}

template <typename T, bool LOSS> void ml_launch(const umr_ml_image* images, int n_images, int R, int C, int M, int max_h, int max_w,
                                                const void* logits, const int64_t* classes, const float* weights, float inv_n,
                                                uint8_t* targets, void* grad, Partial* partials, hipStream_t s) {
    const int lds = (int)ml_lds_bytes(M, max_h, max_w);
    UMR_SET_MAX_LDS_ONCE((ml_main_kernel<T, LOSS>), (int)ML_MAX_LDS);
    ml_main_kernel<T, LOSS><<<dim3(R, ml_slices(M)), ML_THREADS, lds, s>>>(images, n_images, R, C, M, max_h, max_w, (const T*)logits, classes, weights, inv_n,
                                                       targets, (T*)grad, partials);
}

}  // namespace

extern "C" int64_t umr_mask_loss_workspace(int64_t R, int M) {
    if (R < 0 || M < 1 || M > ML_MAX_SIDE) return -1;
    return std::max<int64_t>(R, 1) * ml_slices(M) * (int64_t)sizeof(Partial);
}

extern "C" int umr_mask_targets(const umr_ml_image* images, int n_images, int64_t R, int M, int max_h, int max_w, uint8_t* targets,
                                umr_stream_t stream) {
    if (int st = ml_check_common(images, n_images, R, M, max_h, max_w)) return st;
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(targets, "mask_loss: null targets");
    ml_launch<float, false>(images, n_images, (int)R, 1, M, max_h, max_w, nullptr, nullptr, nullptr, 0.f, targets, nullptr, nullptr,
                            (hipStream_t)stream);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_mask_loss(const umr_ml_image* images, int n_images, int64_t R, int C, int M, int max_h, int max_w, const void* logits,
                             int dtype, const int64_t* gt_classes, const float* weights, int phases, uint8_t* targets, void* grad,
                             float* loss, int64_t* counts, void* workspace, int64_t workspace_bytes, umr_stream_t stream) {
    if (int st = ml_check_common(images, n_images, R, M, max_h, max_w)) return st;
    UMR_CHECK_ARG(C >= 1, "mask_loss: the logits need at least one channel");
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "mask_loss: logits must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(phases > 0 && phases < 4, "mask_loss: phases is a mask of 1 (targets, loss terms, gradient), 2 (finish)");
    UMR_CHECK_ARG(loss && counts && workspace, "mask_loss: null pointer");
    UMR_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "mask_loss: workspace not 8-byte aligned");
    UMR_CHECK_ARG(workspace_bytes >= umr_mask_loss_workspace(R, M), "mask_loss: workspace too small");
    UMR_CHECK_ARG(R == 0 || (logits && grad), "mask_loss: null logits or gradient");
    UMR_CHECK_ARG(R == 0 || C == 1 || gt_classes, "mask_loss: more than one channel needs gt_classes");
    hipStream_t s = (hipStream_t)stream;
    Partial* partials = (Partial*)workspace;
    const double n_elements = (double)R * M * M;
    if ((phases & 1) && R > 0) {
        const float inv_n = (float)(1.0 / n_elements);
        if (dtype == UMR_F32)
            ml_launch<float, true>(images, n_images, (int)R, C, M, max_h, max_w, logits, gt_classes, weights, inv_n, targets, grad, partials, s);
        else
            ml_launch<bf16_t, true>(images, n_images, (int)R, C, M, max_h, max_w, logits, gt_classes, weights, inv_n, targets, grad, partials, s);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        ml_finish_kernel<<<1, ML_THREADS, 0, s>>>(partials, R * ml_slices(M), n_elements, loss, counts);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
