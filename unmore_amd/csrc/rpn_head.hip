// The predictors of the RPN head (Detectron2's StandardRPNHead: a 3x3 convolution with ReLU, then the 1x1 `objectness_logits` (A
// channels) and `anchor_deltas` (4A channels) convolutions, the same weights on every pyramid level), forward and backward, on the
// hidden map of ALL levels in one buffer
//   T [M, C], M = sum over the levels of N * H_l * W_l, row m of level l = first_l + (n * H_l + y) * W_l + x       (NHWC, stacked)
// written straight to / read straight from the per-level NCHW maps that rpn.hip and rpn_loss.hip take in place:
//   logits[l][n, a, y, x] = bo[a] + sum_c T[m, c] * Wo[a, c]          deltas[l][n, j, y, x] = bd[j] + sum_c T[m, c] * Wd[j, c]
//   G[m, c] = (T[m, c] > 0) * sum_{j < 5A} g[m, j] * W[j, c]          (written over T; g = dlogits | ddeltas, W = Wo | Wd stacked)
//   dW[j, c] = sum_m g[m, j] * T[m, c],   db[j] = sum_m g[m, j]
// 5A <= 15 output channels are one 16-wide matrix-core tile.  A wave works on tiles of 16 consecutive rows of T; lane l = 16 q + r reads
// the 16 bytes T[m0 + r][K s + V q .. + V) of step s (V = 8 bf16 / 4 f32 elements, K = 4 V channels per step): T is read once, with
// 16-byte loads, and that fragment IS a matrix-core operand with the row on the tile index and the channel on the sum index -- bf16:
// v_mfma_f32_16x16x32_bf16; f32: four v_mfma_f32_16x16x4_f32, number i of them summing over the channels V q + i.
//
//   rh_predict_kernel   D[j][pixel] = W . T^T: the weights (rounded to the compute type, in LDS) are the A operand, T's fragment the B
//                       operand, so a lane ends with ONE pixel and four output channels, and 16 lanes store 16 consecutive pixels of a
//                       channel.  A tile may straddle an image or a level: every lane finds its own pixel's level, image and offset.
//   rh_bwd_kernel       per pair of tiles (32 rows) and step:  G = W^T . g with the channels of a lane's own fragment on the result's
//                       rows (bf16: two products, whose rows are the channels 8 q' + 4 h + k, so that a lane holds the same 8 channels
//                       of the same pixel as its fragment), masked by T > 0 and stored over the fragment's 16 bytes;  T's tile
//                       transposed by a product with a 0/1 selection matrix (exact: every result is one input times 1 plus zeros), which
//                       leaves a lane with FOUR CONSECUTIVE PIXELS of one channel in its registers -- the sum index of the weight
//                       gradient;  dW[j][c] += g^T . T with g read as four consecutive pixels of a channel of the NCHW map.  The
//                       weight-gradient tile stays in registers over all of the wave's rows, up to 256 channels at a time (more channels:
//                       the rows are walked once per group); all of a pair's loads are issued before its first store; the four waves' sums meet in LDS in wave order: one partial [16][C + 1]
//                       per workgroup (column C: db).
//   finish_partials.h   adds the partials in a fixed order.
// The grid of the backward is min(ceil(M / 128), 512) workgroups, a function of M alone; no float atomics: the same input gives the
// same bytes on every run and every device.
//
// Rounding.  The weights are rounded to the compute type before the products (bf16 compute: bf16 weights).  With bf16 compute the
// incoming gradients g are ROUNDED TO bfloat16 to feed the matrix cores, in G and in dW alike, also when they arrive as float32; db sums
// them unrounded.  With f32 compute nothing is rounded: the f32 matrix-core products are exact f32 fma chains.
#include "finish_partials.h"
#include <algorithm>

namespace {

constexpr int RH_THREADS = 256;
constexpr int RH_MAX_C = 1024;
constexpr int RH_MAX_A = 3;
constexpr int RH_MAX_LEVELS = 8;
constexpr int RH_MAX_WG = 512;              // workgroups of the backward, whatever the device
constexpr int RH_MINW = 2;                 // waves per SIMD the backward is compiled for: two hide each other's load latency (measured: 0.50 ms against 0.56 with one)

struct RhTable {                            // by value in the kernel arguments, copied to LDS: lanes index it by their own level
    int nl;
    int first[RH_MAX_LEVELS];               // first row of the level in T
    int hw[RH_MAX_LEVELS];                  // H * W
    const char* p0[RH_MAX_LEVELS];          // logits / dlogits [N, A, H, W]
    const char* p1[RH_MAX_LEVELS];          // deltas / ddeltas [N, 4A, H, W]
};

struct RhLoc { int lvl, n, yx, hw; };

__device__ __forceinline__ f32x4 rh_mma(f32x4 acc, bf16x8 a, bf16x8 b) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x4 rh_mma(f32x4 acc, f32x4 a, f32x4 b) {      // sum index of product i: lane group q <-> element i
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ void rh_stage_table(RhTable* lds, const RhTable& tab) {
    if (threadIdx.x == 0) {
        lds->nl = tab.nl;
#pragma unroll
        for (int k = 0; k < RH_MAX_LEVELS; ++k) {
            lds->first[k] = tab.first[k]; lds->hw[k] = tab.hw[k]; lds->p0[k] = tab.p0[k]; lds->p1[k] = tab.p1[k];
        }
    }
}

__device__ __forceinline__ RhLoc rh_locate(const RhTable* t, int64_t m) {
    int l = 0;
    for (int k = 1; k < t->nl; ++k)
        if (m >= t->first[k]) l = k;
    RhLoc o;
    o.lvl = l; o.hw = t->hw[l];
    const int local = (int)(m - t->first[l]);
    o.n = local / o.hw;
    o.yx = local - o.n * o.hw;
    return o;
}

// element offset of output channel j (j < A: the logits map; else the deltas map) at a located pixel
__device__ __forceinline__ int64_t rh_offset(const RhLoc& c, int j, int A) {
    return j < A ? ((int64_t)c.n * A + j) * c.hw + c.yx : ((int64_t)c.n * 4 * A + (j - A)) * c.hw + c.yx;
}

__device__ __forceinline__ float rh_grad(const RhTable* t, const RhLoc& c, int j, int A, int g_f32) {
    const char* p = j < A ? t->p0[c.lvl] : t->p1[c.lvl];
    const int64_t o = rh_offset(c, j, A);
    return g_f32 ? ((const float*)p)[o] : (float)((const bf16_t*)p)[o];
}

__device__ __forceinline__ float rh_weight(const float* wo, const float* wd, int j, int c, int C, int A) {
    return j < A ? wo[(int64_t)j * C + c] : (j < 5 * A ? wd[(int64_t)(j - A) * C + c] : 0.f);
}

// dynamic LDS: [16][C + V] weights in the compute type (rows padded by 16 bytes), then the level table
template <typename T>
__global__ __launch_bounds__(RH_THREADS) void rh_predict_kernel(const T* __restrict__ Tm, RhTable tab, int64_t M, int C, int A,
                                                                const float* __restrict__ wo, const float* __restrict__ bo,
                                                                const float* __restrict__ wd, const float* __restrict__ bd, int out_f32) {
    constexpr int V = Chunk16<T>::V, K = 4 * V;
    typedef typename Chunk16<T>::raw raw;
    extern __shared__ __attribute__((aligned(16))) char rh_smem[];
    T* Wl = (T*)rh_smem;
    const int ldw = C + V;
    RhTable* lt = (RhTable*)(rh_smem + (size_t)16 * ldw * sizeof(T));
    rh_stage_table(lt, tab);
    for (int i = threadIdx.x; i < 16 * C; i += RH_THREADS) {
        const int j = i / C, c = i - j * C;
        Wl[j * ldw + c] = from_f32<T>(rh_weight(wo, wd, j, c, C, A));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    float bias[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * q + k;
        bias[k] = j < A ? bo[j] : (j < 5 * A ? bd[j - A] : 0.f);
    }
    const T* wrow = Wl + r * ldw + V * q;
    const int steps = C / K;
    const int64_t ntiles = (M + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * (RH_THREADS / 64) + wv; tile < ntiles; tile += (int64_t)gridDim.x * (RH_THREADS / 64)) {
        const int64_t m = tile * 16 + r;
        const bool valid = m < M;
        const T* row = Tm + (valid ? m : M - 1) * C + V * q;             // a lane past the end reads the last row and stores nothing
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int s = 0;
        for (; s + 4 <= steps; s += 4) {                                 // four loads in flight
            raw f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = *(const raw*)(row + (s + u) * K);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = rh_mma(acc, *(const raw*)(wrow + (s + u) * K), f[u]);
        }
        if (s < steps) {                                                 // C is a multiple of 64: an even number of steps
            const raw f0 = *(const raw*)(row + s * K), f1 = *(const raw*)(row + (s + 1) * K);
            acc = rh_mma(acc, *(const raw*)(wrow + s * K), f0);
            acc = rh_mma(acc, *(const raw*)(wrow + (s + 1) * K), f1);
        }
        if (valid) {
            const RhLoc c = rh_locate(lt, m);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * q + k;
                if (j < 5 * A) {
                    char* p = (char*)(j < A ? lt->p0[c.lvl] : lt->p1[c.lvl]);
                    const int64_t o = rh_offset(c, j, A);
                    const float v = acc[k] + bias[k];
                    if (out_f32) ((float*)p)[o] = v; else ((T*)p)[o] = from_f32<T>(v);
                }
            }
        }
    }
}

// GC: the channels whose weight-gradient tile a wave keeps in registers (64, 128 or 256; C is a multiple of it).
// dynamic LDS: [GC][16] weights of the group, transposed, in the compute type; [16][GC] f32 sums; [4][64] f32 bias sums; the level table
template <typename T, int GC>
__global__ __launch_bounds__(RH_THREADS, RH_MINW) void rh_bwd_kernel(T* __restrict__ Tm, RhTable tab, int64_t M, int C, int A, int g_f32,
                                                            const float* __restrict__ wo, const float* __restrict__ wd,
                                                            float* __restrict__ partials) {
    constexpr int V = Chunk16<T>::V, K = 4 * V, STEPS = GC / K, NB = GC / 16, H = sizeof(T) == 2 ? 2 : 1;
    typedef typename Chunk16<T>::raw raw;
    extern __shared__ __attribute__((aligned(16))) char rh_smem[];
    T* WT = (T*)rh_smem;
    float* sums = (float*)(rh_smem + (size_t)GC * 16 * sizeof(T));
    float* bsum = sums + 16 * GC;
    RhTable* lt = (RhTable*)(bsum + RH_THREADS);
    rh_stage_table(lt, tab);
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 15, q = lane >> 4;
    const int A5 = 5 * A;
    // the selection matrices of the transposing product: B[k][col = r] = 1 where the fragment's channel k is the one column r takes
    raw sel[H];
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int i = 0; i < V; ++i) sel[h][i] = from_f32<T>((V * q + i == 16 * h + r) ? 1.f : 0.f);
    const int64_t npairs = (M + 31) / 32;
    const int64_t stride = (int64_t)gridDim.x * (RH_THREADS / 64);
    float bacc = 0.f;                                                    // lane (j = r, q): sum of its g over the wave's rows
    float* part = partials + (int64_t)blockIdx.x * 16 * (C + 1);
    for (int base = 0; base < C; base += GC) {
        __syncthreads();                                                 // the table, or the previous group's readers of WT and sums
        for (int i = tid; i < GC * 16; i += RH_THREADS) {
            const int c = i >> 4, j = i & 15;
            WT[i] = from_f32<T>(rh_weight(wo, wd, j, base + c, C, A));
        }
        __syncthreads();
        f32x4 accw[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) accw[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t pair = (int64_t)blockIdx.x * (RH_THREADS / 64) + wv; pair < npairs; pair += stride) {
            // g as the B operand of G: lane (pixel r of tile t, q) holds the channels j = V q + i; as the A operand of dW: lane (j = r, q)
            // holds the pixels 4 q + k of tile t
            raw gb[2];
            float ga[2][4];
            bool valid[2];
            raw f[2][STEPS];                                             // every load of the pair before its first store: nothing waits on a store
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int64_t m = (pair * 2 + t) * 16 + r;
                const T* at = Tm + m * C + base + V * q;
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
#pragma unroll
                    for (int i = 0; i < V; ++i) f[t][s][i] = from_f32<T>(0.f);
                    if (m < M) f[t][s] = *(const raw*)(at + s * K);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int64_t m = (pair * 2 + t) * 16 + r;
                valid[t] = m < M;
                float v[V];
#pragma unroll
                for (int i = 0; i < V; ++i) v[i] = 0.f;
                if (valid[t] && V * q < A5) {
                    const RhLoc c = rh_locate(lt, m);
#pragma unroll
                    for (int i = 0; i < V; ++i)
                        if (V * q + i < A5) v[i] = rh_grad(lt, c, V * q + i, A, g_f32);
                }
#pragma unroll
                for (int i = 0; i < V; ++i) gb[t][i] = from_f32<T>(v[i]);
                const int64_t m4 = (pair * 2 + t) * 16 + 4 * q;
#pragma unroll
                for (int k = 0; k < 4; ++k) ga[t][k] = 0.f;
                if (r < A5 && m4 < M) {
                    const RhLoc c = rh_locate(lt, m4);
                    if (m4 + 3 < M && c.yx + 3 < c.hw) {                 // four pixels of one image: consecutive in the NCHW map
                        const char* p = r < A ? lt->p0[c.lvl] : lt->p1[c.lvl];
                        const int64_t o = rh_offset(c, r, A);
#pragma unroll
                        for (int k = 0; k < 4; ++k) ga[t][k] = g_f32 ? ((const float*)p)[o + k] : (float)((const bf16_t*)p)[o + k];
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (m4 + k < M) ga[t][k] = rh_grad(lt, rh_locate(lt, m4 + k), r, A, g_f32);
                    }
                }
                if (base == 0) bacc += (ga[t][0] + ga[t][1]) + (ga[t][2] + ga[t][3]);
            }
            raw gat[2];                                                  // bf16: gat[0] holds both tiles, k = 8 q + i <-> tile i >> 2, pixel 4 q + (i & 3)
            if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int i = 0; i < 8; ++i) gat[0][i] = (bf16_t)ga[i >> 2][i & 3];
                gat[1] = gat[0];
            } else {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int k = 0; k < 4; ++k) gat[t][k] = ga[t][k];
            }
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                f32x4 x[2][H];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    T* at = Tm + ((pair * 2 + t) * 16 + r) * C + base + s * K + V * q;
                    f32x4 g[H];
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        raw w;
                        if constexpr (sizeof(T) == 2) {                  // row r of the product <-> channel 8 (r >> 2) + 4 h + (r & 3) of the step
                            w = *(const raw*)(WT + (s * K + 8 * (r >> 2) + 4 * h + (r & 3)) * 16 + 8 * (q & 1));
                            if (q >= 2) {
#pragma unroll
                                for (int i = 0; i < 8; ++i) w[i] = from_f32<T>(0.f);
                            }
                        } else {
                            w = *(const raw*)(WT + (s * K + r) * 16 + 4 * q);
                        }
                        g[h] = rh_mma(z, w, gb[t]);
                        x[t][h] = rh_mma(z, f[t][s], sel[h]);
                    }
                    if (valid[t]) {
                        raw o;
#pragma unroll
                        for (int i = 0; i < V; ++i) {
                            const float gv = H == 2 ? g[(i >> 2) & (H - 1)][i & 3] : g[0][i & 3];
                            o[i] = (float)f[t][s][i] > 0.f ? from_f32<T>(gv) : from_f32<T>(0.f);
                        }
                        *(raw*)at = o;
                    }
                }
                if constexpr (sizeof(T) == 2) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        bf16x8 xb;
#pragma unroll
                        for (int i = 0; i < 8; ++i) xb[i] = (bf16_t)x[i >> 2][h][i & 3];     // exact: the values are T's own
                        accw[2 * s + h] = rh_mma(accw[2 * s + h], gat[0], xb);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < 2; ++t) accw[s] = rh_mma(accw[s], gat[t], x[t][0]);
                }
            }
        }
        // lane (channel 16 b + r of the group, q) holds the rows j = 4 q + k: the four waves' sums, wave after wave
        for (int w = 0; w < RH_THREADS / 64; ++w) {
            if (wv == w) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float* p = sums + (4 * q + k) * GC + 16 * b + r;
                        *p = w == 0 ? accw[b][k] : *p + accw[b][k];
                    }
            }
            __syncthreads();
        }
        for (int i = tid; i < 16 * GC; i += RH_THREADS) {
            const int j = i / GC, c = i - j * GC;
            part[(int64_t)j * (C + 1) + base + c] = sums[i];
        }
    }
    bsum[tid] = bacc;
    __syncthreads();
    if (tid < 16) {                                                      // j = tid: the lanes (r = j, q) of every wave, in wave then q order
        float s = 0.f;
        for (int w = 0; w < RH_THREADS / 64; ++w)
            for (int k = 0; k < 4; ++k) s += bsum[w * 64 + 16 * k + tid];
        part[(int64_t)tid * (C + 1) + C] = s;
    }
}

struct RhStore {                            // element e of the first 5A rows of a record [16][C + 1]: row j < A of dwo | dbo, else of dwd | dbd
    float *dwo, *dbo, *dwd, *dbd;
    int C, A;
    __device__ void operator()(int e, float v) const {
        const int j = e / (C + 1), c = e - j * (C + 1);
        if (j < A) { if (c < C) dwo[j * C + c] = v; else dbo[j] = v; }
        else { if (c < C) dwd[(j - A) * C + c] = v; else dbd[j - A] = v; }
    }
};

inline int rh_grid(int64_t M) { return (int)std::min<int64_t>(std::max<int64_t>((M + 127) / 128, 1), RH_MAX_WG); }

bool rh_shape_ok(int C, int A) { return C >= 64 && C % 64 == 0 && C <= RH_MAX_C && A >= 1 && A <= RH_MAX_A; }

// checks the arguments and fills the table; *M_out = the rows of T
int rh_table(const int64_t* levels, int n_levels, int64_t N, int C, int A, int dtype, RhTable* tab, int64_t* M_out) {
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "rpn_head: the compute type must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(levels != nullptr && N >= 0, "rpn_head: null level table or negative N");
    if (n_levels < 1 || n_levels > RH_MAX_LEVELS) return umr_set_error(UMR_ERR_UNSUPPORTED, "rpn_head: between 1 and 8 levels");
    if (!rh_shape_ok(C, A))
        return umr_set_error(UMR_ERR_UNSUPPORTED, "rpn_head: C must be a multiple of 64, at most 1024, and 1 <= A <= 3 (5A <= 16)");
    int64_t M = 0;
    *tab = RhTable{};
    tab->nl = n_levels;
    for (int k = 0; k < n_levels; ++k) {
        const int64_t H = levels[4 * k], W = levels[4 * k + 1];
        UMR_CHECK_ARG(H >= 1 && W >= 1 && H <= INT_MAX / W, "rpn_head: a level's H and W must be positive with H * W < 2^31");
        UMR_CHECK_ARG(N == 0 || (levels[4 * k + 2] != 0 && levels[4 * k + 3] != 0), "rpn_head: null map pointer");
        tab->first[k] = (int)M;
        tab->hw[k] = (int)(H * W);
        tab->p0[k] = (const char*)(uintptr_t)levels[4 * k + 2];
        tab->p1[k] = (const char*)(uintptr_t)levels[4 * k + 3];
        UMR_CHECK_ARG(N <= ((int64_t)INT_MAX - M) / (H * W), "rpn_head: M = sum of N * H * W must be below 2^31");
        M += N * H * W;
    }
    for (int k = n_levels; k < RH_MAX_LEVELS; ++k) { tab->first[k] = INT_MAX; tab->hw[k] = 1; }
    *M_out = M;
    return UMR_OK;
}

template <typename T>
void rh_predict_launch(const void* Tm, const RhTable& tab, int64_t M, int C, int A, const float* wo, const float* bo, const float* wd,
                       const float* bd, int out_f32, hipStream_t s) {
    const int lds = 16 * (C + Chunk16<T>::V) * (int)sizeof(T) + (int)sizeof(RhTable);
    UMR_SET_MAX_LDS_ONCE((rh_predict_kernel<T>), 16 * (RH_MAX_C + Chunk16<T>::V) * (int)sizeof(T) + (int)sizeof(RhTable));
    const int64_t tiles = (M + 15) / 16;
    const int blocks = (int)std::min<int64_t>((tiles + 3) / 4, 4096);
    rh_predict_kernel<T><<<blocks, RH_THREADS, lds, s>>>((const T*)Tm, tab, M, C, A, wo, bo, wd, bd, out_f32);
}

template <typename T, int GC>
void rh_bwd_launch_gc(void* Tm, const RhTable& tab, int64_t M, int C, int A, int g_f32, const float* wo, const float* wd,
                      float* partials, hipStream_t s) {
    const int lds = GC * 16 * (int)sizeof(T) + (16 * GC + RH_THREADS) * (int)sizeof(float) + (int)sizeof(RhTable);
    rh_bwd_kernel<T, GC><<<rh_grid(M), RH_THREADS, lds, s>>>((T*)Tm, tab, M, C, A, g_f32, wo, wd, partials);
}

template <typename T>
void rh_bwd_launch(void* Tm, const RhTable& tab, int64_t M, int C, int A, int g_f32, const float* wo, const float* wd, float* partials,
                   hipStream_t s) {
    // bf16: 256 channels per pass measured fastest (0.50 ms at the recipe's shape against 0.59 with 128 and 0.94 with 64); f32 fragments
    // hold half as many channels, so 128 is what fits two waves per SIMD
    if (C % 256 == 0 && sizeof(T) == 2) rh_bwd_launch_gc<T, 256>(Tm, tab, M, C, A, g_f32, wo, wd, partials, s);
    else if (C % 128 == 0) rh_bwd_launch_gc<T, 128>(Tm, tab, M, C, A, g_f32, wo, wd, partials, s);
    else rh_bwd_launch_gc<T, 64>(Tm, tab, M, C, A, g_f32, wo, wd, partials, s);
}

}  // namespace

extern "C" int64_t umr_rpn_head_workspace(int64_t M, int C, int A) {
    if (M < 0 || M > INT_MAX || !rh_shape_ok(C, A)) return -1;
    return (int64_t)rh_grid(M) * 16 * (C + 1) * (int64_t)sizeof(float);
}

extern "C" int umr_rpn_head_predict(const void* T, const int64_t* levels, int n_levels, int64_t N, int C, int A, const float* wo,
                                    const float* bo, const float* wd, const float* bd, int dtype, int out_f32, umr_stream_t stream) {
    RhTable tab;
    int64_t M;
    if (int st = rh_table(levels, n_levels, N, C, A, dtype, &tab, &M)) return st;
    if (M == 0) return UMR_OK;
    UMR_CHECK_ARG(T && wo && bo && wd && bd, "rpn_head: null pointer");
    UMR_CHECK_ARG(((uintptr_t)T & 15) == 0, "rpn_head: T must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == UMR_F32) rh_predict_launch<float>(T, tab, M, C, A, wo, bo, wd, bd, out_f32 != 0, s);
    else rh_predict_launch<bf16_t>(T, tab, M, C, A, wo, bo, wd, bd, out_f32 != 0, s);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_rpn_head_predict_bwd(void* T, const int64_t* levels, int n_levels, int64_t N, int C, int A, int grads_f32,
                                        const float* wo, const float* wd, float* dwo, float* dbo, float* dwd, float* dbd,
                                        void* workspace, int64_t workspace_bytes, int dtype, int phases, umr_stream_t stream) {
    RhTable tab;
    int64_t M;
    if (int st = rh_table(levels, n_levels, N, C, A, dtype, &tab, &M)) return st;
    UMR_CHECK_ARG(phases > 0 && phases < 4, "rpn_head: phases is a mask of 1 (G and the partial sums), 2 (the finishing sum)");
    UMR_CHECK_ARG(dwo && dbo && dwd && dbd && workspace, "rpn_head: null pointer");
    UMR_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "rpn_head: workspace not 4-byte aligned");
    UMR_CHECK_ARG(workspace_bytes >= umr_rpn_head_workspace(M, C, A), "rpn_head: workspace too small");
    UMR_CHECK_ARG(M == 0 || (T && wo && wd), "rpn_head: null pointer");
    UMR_CHECK_ARG(((uintptr_t)T & 15) == 0, "rpn_head: T must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* partials = (float*)workspace;
    const int g_f32 = dtype == UMR_F32 || grads_f32 != 0;
    if ((phases & 1) && M > 0) {
        if (dtype == UMR_F32) rh_bwd_launch<float>(T, tab, M, C, A, g_f32, wo, wd, partials, s);
        else rh_bwd_launch<bf16_t>(T, tab, M, C, A, g_f32, wo, wd, partials, s);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        finish_partials_kernel<<<(5 * A * (C + 1) + 63) / 64, FINISH_THREADS, 0, s>>>(partials, M > 0 ? rh_grid(M) : 0, 16 * (C + 1),
                                                                                      5 * A * (C + 1), RhStore{dwo, dbo, dwd, dbd, C, A});
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
