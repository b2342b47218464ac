// The tail of the detector's mask head (CustomMaskRCNNConvUpsampleHead, cad/modeling/roi_heads/roi_heads.py:1098-1201): the 1x1
// predictor on the ReLU'd output of the 2x2 stride-2 deconvolution, forward and backward, straight on the deconvolution GEMM's output
//   D [M, 4C], M = R*S*S, row m = (r*S + y)*S + x, column n = (2*ky + kx)*C + co        (packs._pack_convT's order)
// so that the [R,2S,2S,C] feature map is never laid out:
//   logit[r, 2y+ky, 2x+kx] = bp + sum_co D[m, (ky,kx,co)] * wp[co]
//   G[m, (ky,kx,co)]       = dlogit[r, 2y+ky, 2x+kx] * wp[co] * (D > 0)                   (written over D)
//   dwp[co] = sum_{m,tap} dlogit * D[m, (tap,co)],   dbp = sum dlogit
//
// Both kernels stream D once with 16-byte loads: a wave owns whole rows, lane l holds the chunks l, l + 64, ... of 16 bytes of its row,
// so consecutive lanes read consecutive addresses.  Which tap and which channels a lane's chunk j belongs to is the same for every
// row: the predictor's weights of those channels sit in registers for the whole launch.
//
//   mh_logits_kernel   per chunk a dot product in channel order, per lane one sum per tap in chunk order, then one butterfly that
//                      folds the four sums and the 64 lanes together (7 exchanges: the halves of the wave keep two taps each, the quarters one).  The order of the
//                      additions is a function of C and the element size alone.
//   mh_tail_bwd_kernel a workgroup of four waves owns 256 rows, a wave 64 of them in turn.  Lane l reads the four dlogits of the wave's row l
//                      once; a row's four values reach the other lanes as wave-uniform registers.  Every lane adds dlogit * D to
//                      the sums of its own chunks over the wave's rows; the four waves' sums meet in LDS, wave after wave, then
//                      the four taps of a channel, in tap order: one f32 partial per channel and workgroup, the workgroup's sum of dlogits after them.
//   finish_partials.h  adds the workgroups' partials in a fixed order.  No float atomics anywhere: the same input gives the same bytes on every run.
#include "finish_partials.h"
#include <algorithm>

namespace {

constexpr int MH_THREADS = 256;
constexpr int MH_ROWS = 256;               // rows of D per workgroup of the backward kernel: 64 per wave
constexpr int MH_MAX_C = 1024;
constexpr int MH_MAX_S = 64;

__device__ __forceinline__ float mh_uniform(float v, int lane) {        // lane `lane` (wave-uniform) of v, as a wave-uniform value
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One sum per tap and lane -> the sum over the wave of tap (lane >> 4), in every lane.
__device__ __forceinline__ float mh_fold_taps(float a0, float a1, float a2, float a3, int lane) {
    const bool up = (lane & 32) != 0;
    const float k0 = (up ? a2 : a0) + __shfl_xor(up ? a0 : a2, 32, 64);
    const float k1 = (up ? a3 : a1) + __shfl_xor(up ? a1 : a3, 32, 64);
    const bool up2 = (lane & 16) != 0;
    float k = (up2 ? k1 : k0) + __shfl_xor(up2 ? k0 : k1, 16, 64);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
    return k;
}

// NP: the passes of 64 chunks a row takes, rounded up to one of the instantiated counts; a chunk past the row's end is skipped.
template <typename T, int NP>
__global__ __launch_bounds__(MH_THREADS) void mh_logits_kernel(const T* __restrict__ D, const float* __restrict__ wp,
                                                               const float* __restrict__ bp, void* __restrict__ out, int64_t M, int S,
                                                               int C, int out_f32, int sigmoid) {
    typedef Chunk16<T> CH;
    constexpr int V = CH::V;
    const int lane = threadIdx.x & 63;
    const int row_elems = 4 * C;
    float w[NP][V];
    int tap[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int e = (lane + 64 * j) * V;
        tap[j] = e < row_elems ? e / C : -1;
#pragma unroll
        for (int v = 0; v < V; ++v) w[j][v] = e < row_elems ? wp[e % C + v] : 0.f;
    }
    const float bias = bp[0];
    const int S2 = 2 * S;
    const int64_t waves = (int64_t)gridDim.x * (MH_THREADS / 64);
    for (int64_t m = (int64_t)blockIdx.x * (MH_THREADS / 64) + (threadIdx.x >> 6); m < M; m += waves) {
        const T* row = D + m * row_elems;
        typename CH::raw d[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (tap[j] >= 0) d[j] = *(const typename CH::raw*)(row + (lane + 64 * j) * V);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (tap[j] < 0) continue;
            float s = 0.f;
#pragma unroll
            for (int v = 0; v < V; ++v) s += CH::get(d[j], v) * w[j][v];
            a0 += tap[j] == 0 ? s : 0.f;
            a1 += tap[j] == 1 ? s : 0.f;
            a2 += tap[j] == 2 ? s : 0.f;
            a3 += tap[j] == 3 ? s : 0.f;
        }
        const float sum = mh_fold_taps(a0, a1, a2, a3, lane);
        if ((lane & 15) == 0) {
            const int t = lane >> 4;
            const int64_t r = m / (S * S);
            const int yx = (int)(m - r * (S * S)), y = yx / S, x = yx - y * S;
            const int64_t o = (r * S2 + (2 * y + (t >> 1))) * S2 + 2 * x + (t & 1);
            float val = bias + sum;
            if (sigmoid) val = (float)(1.0 / (1.0 + exp(-(double)val)));
            if (out_f32) ((float*)out)[o] = val; else ((T*)out)[o] = from_f32<T>(val);
        }
    }
}

__device__ __forceinline__ float mh_dlogit(const void* dl, int dl_f32, int64_t i) {
    return dl_f32 ? ((const float*)dl)[i] : (float)((const bf16_t*)dl)[i];
}

template <typename T, int NP>
__global__ __launch_bounds__(MH_THREADS) void mh_tail_bwd_kernel(T* __restrict__ D, const void* __restrict__ dlogits, int dl_f32,
                                                                 const float* __restrict__ wp, float* __restrict__ partials, int64_t M,
                                                                 int S, int C) {
    typedef Chunk16<T> CH;
    constexpr int V = CH::V;
    extern __shared__ __attribute__((aligned(16))) float mh_sums[];      // [4 * C] the workgroup's sums per column of D, then [4] dlogit sums
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row_elems = 4 * C;
    float w[NP][V], acc[NP][V];
    int tap[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int e = (lane + 64 * j) * V;
        tap[j] = e < row_elems ? e / C : -1;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            w[j][v] = e < row_elems ? wp[e % C + v] : 0.f;
            acc[j][v] = 0.f;
        }
    }
    // the four dlogits of row (first + lane)
    const int S2 = 2 * S;
    const int64_t first = (int64_t)blockIdx.x * MH_ROWS + wv * 64;
    const int nrows = (int)std::min<int64_t>(64, std::max<int64_t>(M - first, 0));
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane < nrows) {
        const int64_t m = first + lane, r = m / (S * S);
        const int yx = (int)(m - r * (S * S)), y = yx / S, x = yx - y * S;
        const int64_t o = (r * S2 + 2 * y) * S2 + 2 * x;
        if constexpr (sizeof(T) == 4) {
            g[0] = ((const float*)dlogits)[o]; g[1] = ((const float*)dlogits)[o + 1];
            g[2] = ((const float*)dlogits)[o + S2]; g[3] = ((const float*)dlogits)[o + S2 + 1];
        } else {
            g[0] = mh_dlogit(dlogits, dl_f32, o); g[1] = mh_dlogit(dlogits, dl_f32, o + 1);
            g[2] = mh_dlogit(dlogits, dl_f32, o + S2); g[3] = mh_dlogit(dlogits, dl_f32, o + S2 + 1);
        }
    }
    for (int i0 = 0; i0 < nrows; i0 += 2) {                                // wave-uniform; two rows' loads in flight
        const int nr = std::min(2, nrows - i0);
        typename CH::raw d[2][NP];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < NP; ++j)
                if (u < nr && tap[j] >= 0) d[u][j] = *(const typename CH::raw*)(D + (first + i0 + u) * row_elems + (lane + 64 * j) * V);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u >= nr) break;
            const int i = i0 + u;
            T* row = D + (first + i) * row_elems;
            const float g0 = mh_uniform(g[0], i), g1 = mh_uniform(g[1], i), g2 = mh_uniform(g[2], i), g3 = mh_uniform(g[3], i);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                if (tap[j] < 0) continue;
                const float gl = tap[j] == 0 ? g0 : tap[j] == 1 ? g1 : tap[j] == 2 ? g2 : g3;
                typename CH::raw o;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float x = CH::get(d[u][j], v);
                    acc[j][v] += gl * x;
                    CH::set(o, v, x > 0.f ? gl * w[j][v] : 0.f);
                }
                *(typename CH::raw*)(row + (lane + 64 * j) * V) = o;
            }
        }
    }
    // the four waves' sums, wave after wave
    for (int k = 0; k < MH_THREADS / 64; ++k) {
        if (wv == k) {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                if (tap[j] < 0) continue;
                float* p = mh_sums + (lane + 64 * j) * V;
#pragma unroll
                for (int v = 0; v < V; ++v) p[v] = k == 0 ? acc[j][v] : p[v] + acc[j][v];
            }
        }
        __syncthreads();
    }
    const float gs = wave_sum((g[0] + g[1]) + (g[2] + g[3]));
    if (lane == 0) mh_sums[row_elems + wv] = gs;
    __syncthreads();
    float* part = partials + (int64_t)blockIdx.x * (C + 1);
    for (int c = tid; c < C; c += MH_THREADS) part[c] = ((mh_sums[c] + mh_sums[C + c]) + mh_sums[2 * C + c]) + mh_sums[3 * C + c];
    if (tid == 0) part[C] = ((mh_sums[row_elems] + mh_sums[row_elems + 1]) + mh_sums[row_elems + 2]) + mh_sums[row_elems + 3];
}

struct MhStore {                            // element c of a record [C + 1]: dwp[c], then dbp
    float *dwp, *dbp;
    int C;
    __device__ void operator()(int c, float v) const { if (c < C) dwp[c] = v; else dbp[0] = v; }
};

inline int64_t mh_blocks(int64_t M) { return (M + MH_ROWS - 1) / MH_ROWS; }

template <typename T> int mh_passes(int C) { return (4 * C / Chunk16<T>::V + 63) / 64; }

int mh_check(int64_t R, int S, int C, int dtype) {
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "mask_head: the compute type must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(R >= 0, "mask_head: negative R");
    if (C < 64 || C % 64 != 0 || C > MH_MAX_C)
        return umr_set_error(UMR_ERR_UNSUPPORTED, "mask_head: C must be a multiple of 64, at most 1024");
    if (S < 1 || S > MH_MAX_S) return umr_set_error(UMR_ERR_UNSUPPORTED, "mask_head: S must be in [1, 64]");
    UMR_CHECK_ARG(R <= (int64_t)INT_MAX / (S * S), "mask_head: R * S * S must be below 2^31");
    return UMR_OK;
}

template <typename T, int NP>
void mh_logits_launch(const void* D, const float* wp, const float* bp, void* out, int64_t M, int S, int C, int out_f32, int sigmoid,
                      hipStream_t s) {
    const int64_t blocks = std::min<int64_t>((M + MH_THREADS / 64 - 1) / (MH_THREADS / 64), 8192);
    mh_logits_kernel<T, NP><<<(int)blocks, MH_THREADS, 0, s>>>((const T*)D, wp, bp, out, M, S, C, out_f32, sigmoid);
}

template <typename T, int NP>
void mh_bwd_launch(void* D, const void* dlogits, int dl_f32, const float* wp, float* partials, int64_t M, int S, int C, hipStream_t s) {
    const int lds = (4 * C + 4) * (int)sizeof(float);
    mh_tail_bwd_kernel<T, NP><<<(int)mh_blocks(M), MH_THREADS, lds, s>>>((T*)D, dlogits, dl_f32, wp, partials, M, S, C);
}

// the instantiated pass counts: 1, 2, 4 and the most a row of 4 * 1024 elements takes
#define MH_DISPATCH(T, fn, ...)                                                              \
    do {                                                                                     \
        const int np_ = mh_passes<T>(C);                                                     \
        if (np_ <= 1) fn<T, 1>(__VA_ARGS__);                                                 \
        else if (np_ <= 2) fn<T, 2>(__VA_ARGS__);                                            \
        else if (np_ <= 4) fn<T, 4>(__VA_ARGS__);                                            \
        else fn<T, 4 * MH_MAX_C / Chunk16<T>::V / 64>(__VA_ARGS__);                          \
    } while (0)

}  // namespace

extern "C" int64_t umr_mask_head_workspace(int64_t M, int C) {
    if (M < 0 || M > INT_MAX || C < 64 || C % 64 != 0 || C > MH_MAX_C) return -1;
    return std::max<int64_t>(mh_blocks(M), 1) * (C + 1) * (int64_t)sizeof(float);
}

extern "C" int umr_mask_head_logits(const void* D, const float* wp, const float* bp, void* logits, int64_t R, int S, int C, int dtype,
                                    int out_f32, int sigmoid, umr_stream_t stream) {
    if (int st = mh_check(R, S, C, dtype)) return st;
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(D && wp && bp && logits, "mask_head: null pointer");
    UMR_CHECK_ARG(((uintptr_t)D & 15) == 0, "mask_head: D must be 16-byte aligned");
    const int64_t M = R * S * S;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == UMR_F32) MH_DISPATCH(float, mh_logits_launch, D, wp, bp, logits, M, S, C, out_f32 != 0, sigmoid != 0, s);
    else MH_DISPATCH(bf16_t, mh_logits_launch, D, wp, bp, logits, M, S, C, out_f32 != 0, sigmoid != 0, s);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_mask_head_tail_bwd(void* D, const void* dlogits, int dlogits_f32, const float* wp, float* dwp, float* dbp,
                                      void* workspace, int64_t workspace_bytes, int64_t R, int S, int C, int dtype, int phases,
                                      umr_stream_t stream) {
    if (int st = mh_check(R, S, C, dtype)) return st;
    UMR_CHECK_ARG(phases > 0 && phases < 4, "mask_head: phases is a mask of 1 (G and the partial sums), 2 (the finishing sum)");
    UMR_CHECK_ARG(dwp && dbp && workspace, "mask_head: null pointer");
    UMR_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "mask_head: workspace not 4-byte aligned");
    const int64_t M = R * S * S;
    UMR_CHECK_ARG(workspace_bytes >= umr_mask_head_workspace(M, C), "mask_head: workspace too small");
    UMR_CHECK_ARG(R == 0 || (D && dlogits && wp), "mask_head: null pointer");
    UMR_CHECK_ARG(((uintptr_t)D & 15) == 0, "mask_head: D must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* partials = (float*)workspace;
    const int dl_f32 = dtype == UMR_F32 || dlogits_f32 != 0;
    if ((phases & 1) && R > 0) {
        if (dtype == UMR_F32) MH_DISPATCH(float, mh_bwd_launch, D, dlogits, dl_f32, wp, partials, M, S, C, s);
        else MH_DISPATCH(bf16_t, mh_bwd_launch, D, dlogits, dl_f32, wp, partials, M, S, C, s);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        finish_partials_kernel<<<(C + 1 + 63) / 64, FINISH_THREADS, 0, s>>>(partials, R > 0 ? mh_blocks(M) : 0, C + 1, C + 1,
                                                                            MhStore{dwp, dbp, C});
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
