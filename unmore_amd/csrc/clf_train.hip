// Training-mode pieces of the existence classifier (train_objectness_net.py:540-743, BinaryClassifierTrainer: torchvision
// ResNet-50 + Linear(1000,1) + sigmoid under BCELoss, model.train()).  The convolutions, their data / weight gradients and the
// Linear layers run on umr_gemm_nt / umr_gemm_tn (unmore_amd/classifier_trainer.py chains them); what is left is HBM-bound:
//   umr_bn_train_stats          batch statistics of a raw conv output (+ running statistics, num_batches_tracked)
//   umr_bn_train_apply          y = act(bn(z) [+ bn2(z2) | + residual])
//   umr_bn_train_bwd_reduce     dgamma / dbeta (= the two sums the input gradient needs)
//   umr_bn_train_bwd_apply      dz of one or two BatchNorms fed by the same gradient
//   umr_maxpool3x3s2_bwd        gather-form gradient of the stem's max-pool
//   umr_stuff2_add              stride-2 shortcut: data gradient of the 1x1 s2 conv added at the even positions
//   umr_bce_sigmoid             BCELoss(sigmoid(logit)) and d loss / d logit
// Layout NHWC ([M rows][C channels]), four channels per thread.  The reductions split the rows into a fixed number of chunks
// (a function of M and C only) and combine the per-chunk partials in a fixed order: bitwise reproducible, no float atomics.
#include "umr_common.h"

namespace {

constexpr int kTileC = 64;          // channels per block of the column reductions (16 threads x 4)
constexpr int kRowLanes = 16;       // rows in flight per block of the column reductions

int bn_chunks(int M, int C) {
    const int ctiles = (C + kTileC - 1) / kTileC;
    int ch = 1024 / ctiles;
    const int maxch = (M + 63) / 64;   // >= 4 rows per thread
    if (ch > maxch) ch = maxch;
    return ch < 1 ? 1 : ch;
}

int grid_cap(int64_t total, int block = 256, int cap = 65536) {
    int64_t g = (total + block - 1) / block;
    if (g > cap) g = cap;
    return g < 1 ? 1 : (int)g;
}

// LDS: sums of the 16 row lanes of a block for `nq` quantities, in row-lane order -> part[(chunk * stride + k) * C + c]
template <int NQ>
__device__ __forceinline__ void reduce_lanes_to_partials(float (*sh)[kRowLanes][kTileC + 1], const f32x4 (&acc)[NQ], int nq, float* part,
                                                   int stride, int chunk, int C) {
    const int q = threadIdx.x & 15, rl = threadIdx.x >> 4;
    for (int k = 0; k < nq; ++k)
        for (int e = 0; e < 4; ++e) sh[k][rl][q * 4 + e] = acc[k][e];
    __syncthreads();
    for (int t = threadIdx.x; t < nq * kTileC; t += blockDim.x) {
        const int k = t / kTileC, j = t % kTileC;
        float a = 0.f;
        for (int i = 0; i < kRowLanes; ++i) a += sh[k][i][j];
        const int c = blockIdx.x * kTileC + j;
        if (c < C) part[((int64_t)chunk * stride + k) * C + c] = a;
    }
}

// ---------------------------------------------------------------- statistics
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const T* __restrict__ z, float* __restrict__ part, int M, int C, int rpc) {
    __shared__ float sh[2][kRowLanes][kTileC + 1];
    const int q = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * kTileC + q * 4;
    const int chunk = blockIdx.y;
    const int r0 = chunk * rpc, r1 = min(M, r0 + rpc);
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (c < C) {
        const f32x4 k = Vec4<T>::load(z + c);   // shift: row 0 of the channel (a sample, within a few sigma of the mean)
        for (int r = r0 + rl; r < r1; r += kRowLanes) {
            const f32x4 v = Vec4<T>::load(z + (int64_t)r * C + c) - k;
            acc[0] += v;
            acc[1] += v * v;
        }
    }
    reduce_lanes_to_partials<2>(sh, acc, 2, part, 2, chunk, C);
}

// one wave per channel: lane l sums the chunks l, l + 64, ... in order, then a fixed xor tree (wave_sum) combines the lanes
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const T* __restrict__ z, const float* __restrict__ part, int chunks,
                                                             float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ rmean,
                                                             float* __restrict__ rvar, int64_t* __restrict__ nbt, int M, int C, float eps,
                                                             float mom) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt != nullptr) nbt[0] += 1;
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    float s1 = 0.f, s2 = 0.f;
    for (int k = lane; k < chunks; k += 64) {
        s1 += part[(int64_t)(2 * k) * C + c];
        s2 += part[(int64_t)(2 * k + 1) * C + c];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane != 0) return;
    const float n = (float)M;
    const float d = s1 / n;                       // mean - shift
    const float m2 = fmaxf(s2 - s1 * d, 0.f);     // sum (x - mean)^2
    const float mu = to_f32<T>(z[c]) + d;
    mean[c] = mu;
    rstd[c] = 1.0f / sqrtf(m2 / n + eps);
    if (rmean != nullptr) rmean[c] = (1.f - mom) * rmean[c] + mom * mu;
    if (rvar != nullptr) rvar[c] = (1.f - mom) * rvar[c] + mom * (m2 / (n - 1.f));
}

// ---------------------------------------------------------------- apply
template <typename T>
__global__ void bn_apply_kernel(const T* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                const float* __restrict__ gamma, const float* __restrict__ beta, const T* __restrict__ z2,
                                const float* __restrict__ mean2, const float* __restrict__ rstd2, const float* __restrict__ gamma2,
                                const float* __restrict__ beta2, const T* __restrict__ res, T* __restrict__ y, int64_t total4, int C,
                                int act) {
    const int c4 = C >> 2;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4) * 4;
        const int64_t off = idx * 4;
        const f32x4 v = Vec4<T>::load(z + off);
        f32x4 o;
        for (int e = 0; e < 4; ++e) o[e] = gamma[c + e] * ((v[e] - mean[c + e]) * rstd[c + e]) + beta[c + e];
        if (z2 != nullptr) {
            const f32x4 v2 = Vec4<T>::load(z2 + off);
            for (int e = 0; e < 4; ++e) o[e] += gamma2[c + e] * ((v2[e] - mean2[c + e]) * rstd2[c + e]) + beta2[c + e];
        } else if (res != nullptr) {
            o += Vec4<T>::load(res + off);
        }
        if (act == 1)
            for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
        Vec4<T>::store(y + off, o);
    }
}

// ---------------------------------------------------------------- backward
struct BwdArgs {
    const void* dy; const float* dpool; const void* y;
    const void* z[2]; const float* mean[2]; const float* rstd[2]; const float* gamma[2];
    float* dgamma[2]; float* dbeta[2]; void* dz[2]; void* g_out;
    int64_t rpb; float scale; int M, C, nb;
};

template <typename T>
__device__ __forceinline__ f32x4 load_g(const BwdArgs& a, int64_t r, int c) {
    const int64_t off = r * a.C + c;
    f32x4 g;
    if (a.dy != nullptr) {
        g = Vec4<T>::load((const T*)a.dy + off);
    } else {
        g = *(const f32x4*)(a.dpool + (r / a.rpb) * a.C + c);
        g *= a.scale;
    }
    if (a.y != nullptr) {
        const f32x4 yv = Vec4<T>::load((const T*)a.y + off);
        for (int e = 0; e < 4; ++e) g[e] = yv[e] > 0.f ? g[e] : 0.f;
    }
    return g;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(BwdArgs a, float* __restrict__ part, int rpc) {
    __shared__ float sh[3][kRowLanes][kTileC + 1];
    const int q = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * kTileC + q * 4;
    const int chunk = blockIdx.y;
    const int r0 = chunk * rpc, r1 = min(a.M, r0 + rpc);
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (c < a.C) {
        f32x4 mu[2], rs[2];
        for (int b = 0; b < a.nb; ++b) {
            mu[b] = *(const f32x4*)(a.mean[b] + c);
            rs[b] = *(const f32x4*)(a.rstd[b] + c);
        }
        for (int r = r0 + rl; r < r1; r += kRowLanes) {
            const f32x4 g = load_g<T>(a, r, c);
            acc[0] += g;
            for (int b = 0; b < a.nb; ++b) {
                const f32x4 xh = (Vec4<T>::load((const T*)a.z[b] + (int64_t)r * a.C + c) - mu[b]) * rs[b];
                acc[1 + b] += g * xh;
            }
        }
    }
    reduce_lanes_to_partials<3>(sh, acc, 1 + a.nb, part, 3, chunk, a.C);
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(BwdArgs a, const float* __restrict__ part, int chunks) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);     // one wave per channel, as bn_stats_final_kernel
    if (c >= a.C) return;
    float s[3] = {0.f, 0.f, 0.f};
    for (int k = lane; k < chunks; k += 64)
        for (int j = 0; j <= a.nb; ++j) s[j] += part[(int64_t)(3 * k + j) * a.C + c];
    for (int j = 0; j < 3; ++j) s[j] = wave_sum(s[j]);
    if (lane != 0) return;
    for (int b = 0; b < a.nb; ++b) {
        a.dbeta[b][c] = s[0];
        a.dgamma[b][c] = s[1 + b];
    }
}

template <typename T>
__global__ void bn_bwd_apply_kernel(BwdArgs a) {
    const int c4 = a.C >> 2;
    const int64_t total4 = (int64_t)a.M * c4;
    const float inv_n = 1.0f / (float)a.M;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4) * 4;
        const int64_t r = idx / c4;
        const int64_t off = idx * 4;
        const f32x4 g = load_g<T>(a, r, c);
        for (int b = 0; b < a.nb; ++b) {
            const f32x4 v = Vec4<T>::load((const T*)a.z[b] + off);
            f32x4 o;
            for (int e = 0; e < 4; ++e) {
                const float rs = a.rstd[b][c + e];
                const float xh = (v[e] - a.mean[b][c + e]) * rs;
                o[e] = a.gamma[b][c + e] * rs * (g[e] - a.dbeta[b][c + e] * inv_n - xh * (a.dgamma[b][c + e] * inv_n));
            }
            Vec4<T>::store((T*)a.dz[b] + off, o);
        }
        if (a.g_out != nullptr) Vec4<T>::store((T*)a.g_out + off, g);
    }
}

// ---------------------------------------------------------------- max-pool backward (gather), stride-2 scatter
template <typename T>
__global__ void maxpool3x3s2_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ dx, int B, int H, int W, int C,
                                        int Ho, int Wo) {
    const int c4 = C >> 2;
    const int64_t total = (int64_t)B * H * W * c4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4) * 4;
        int64_t r = idx / c4;
        const int ix = (int)(r % W); r /= W;
        const int iy = (int)(r % H);
        const int b = (int)(r / H);
        const T* xb = x + (int64_t)b * H * W * C + c;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int oy1 = min(Ho - 1, (iy + 1) >> 1), ox1 = min(Wo - 1, (ix + 1) >> 1);
        for (int oy = iy >> 1; oy <= oy1; ++oy) {
            for (int ox = ix >> 1; ox <= ox1; ++ox) {
                // the window's argmax per channel: first maximum in (ky, kx) order; a NaN is taken, as torch takes it
                f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                int arg[4] = {-1, -1, -1, -1};
                for (int ky = 0; ky < 3; ++ky) {
                    const int yy = oy * 2 - 1 + ky;
                    if ((unsigned)yy >= (unsigned)H) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        const int xx = ox * 2 - 1 + kx;
                        if ((unsigned)xx >= (unsigned)W) continue;
                        const f32x4 v = Vec4<T>::load(xb + ((int64_t)yy * W + xx) * C);
                        for (int e = 0; e < 4; ++e)
                            if (arg[e] < 0 || v[e] > m[e] || __builtin_isnan(v[e])) { m[e] = v[e]; arg[e] = ky * 3 + kx; }
                    }
                }
                const int mine = (iy - (oy * 2 - 1)) * 3 + (ix - (ox * 2 - 1));
                const f32x4 g = Vec4<T>::load(dy + (((int64_t)b * Ho + oy) * Wo + ox) * C + c);
                for (int e = 0; e < 4; ++e)
                    if (arg[e] == mine) acc[e] += g[e];
            }
        }
        Vec4<T>::store(dx + idx * 4, acc);
    }
}

template <typename T>
__global__ void stuff2_add_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int H, int W, int Ho, int Wo, int C) {
    const int c4 = C >> 2;
    const int64_t total = (int64_t)B * Ho * Wo * c4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4) * 4;
        int64_t r = idx / c4;
        const int x = (int)(r % Wo); r /= Wo;
        const int y = (int)(r % Ho);
        const int b = (int)(r / Ho);
        T* d = dst + (((int64_t)b * H + 2 * y) * W + 2 * x) * C + c;
        Vec4<T>::store(d, Vec4<T>::load(d) + Vec4<T>::load(src + idx * 4));
    }
}

// ---------------------------------------------------------------- loss
__global__ __launch_bounds__(256) void bce_sigmoid_kernel(const float* __restrict__ logit, const float* __restrict__ label,
                                                          float* __restrict__ loss, float* __restrict__ dlogit, int B) {
    __shared__ float sh[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        const float z = logit[i], y = label[i];
        const float p = 1.0f / (1.0f + expf(-z));
        s += (y - 1.0f) * fmaxf(log1pf(-p), -100.0f) - y * fmaxf(logf(p), -100.0f);
        const float dp = (p - y) / fmaxf((1.0f - p) * p, 1e-12f) / (float)B;   // binary_cross_entropy_backward, mean reduction
        dlogit[i] = dp * (1.0f - p) * p;                                       // sigmoid_backward
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = sh[0] / (float)B;
}

}  // namespace

#define DISPATCH_T(dtype, CALL)                                   \
    if ((dtype) == UMR_BF16) { typedef bf16_t T; CALL; }          \
    else if ((dtype) == UMR_F32) { typedef float T; CALL; }       \
    else return umr_set_error(UMR_ERR_INVALID, "dtype");

extern "C" int64_t umr_bn_train_workspace(int M, int C) {
    if (M <= 0 || C <= 0) return 0;
    return (int64_t)bn_chunks(M, C) * 3 * C * (int64_t)sizeof(float);
}

extern "C" int umr_bn_train_stats(const void* z, float* mean, float* rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                  void* workspace, int64_t workspace_bytes, int M, int C, float eps, float momentum, int dtype,
                                  umr_stream_t stream) {
    UMR_CHECK_ARG(z && mean && rstd && workspace, "bn_train_stats: null pointer");
    UMR_CHECK_ARG(M > 0 && C > 0 && C % 4 == 0, "bn_train_stats: bad geometry (M > 0, C a positive multiple of 4)");
    UMR_CHECK_ARG(!(running_mean || running_var) || M > 1, "bn_train_stats: the running variance needs more than one value per channel");
    UMR_CHECK_ARG(workspace_bytes >= umr_bn_train_workspace(M, C), "bn_train_stats: workspace too small");
    const int chunks = bn_chunks(M, C);
    const int rpc = (M + chunks - 1) / chunks;
    float* part = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL(bn_stats_partial_kernel<T>, dim3((C + kTileC - 1) / kTileC, chunks), dim3(256), 0, s, (const T*)z, part,
                                         M, C, rpc);
               hipLaunchKernelGGL(bn_stats_final_kernel<T>, dim3((C + 3) / 4), dim3(256), 0, s, (const T*)z, (const float*)part, chunks,
                                  mean, rstd, running_mean, running_var, num_batches_tracked, M, C, eps, momentum));
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_bn_train_apply(const void* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* z2,
                                  const float* mean2, const float* rstd2, const float* gamma2, const float* beta2, const void* residual,
                                  void* y, int M, int C, int act, int dtype, umr_stream_t stream) {
    UMR_CHECK_ARG(z && mean && rstd && gamma && beta && y, "bn_train_apply: null pointer");
    UMR_CHECK_ARG(!z2 || (mean2 && rstd2 && gamma2 && beta2), "bn_train_apply: second branch without its statistics / parameters");
    UMR_CHECK_ARG(!(z2 && residual), "bn_train_apply: a second branch or a residual, not both");
    UMR_CHECK_ARG(M > 0 && C > 0 && C % 4 == 0 && (act == 0 || act == 1), "bn_train_apply: bad geometry or act");
    const int64_t total4 = (int64_t)M * (C / 4);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_cap(total4)), dim3(256), 0, s, (const T*)z, mean, rstd, gamma, beta,
                                         (const T*)z2, mean2, rstd2, gamma2, beta2, (const T*)residual, (T*)y, total4, C, act));
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

static int bwd_args(const umr_bn_bwd_desc* d, BwdArgs& a, bool apply) {
    UMR_CHECK_ARG(d != nullptr, "bn_train_bwd: null descriptor");
    UMR_CHECK_ARG(d->M > 0 && d->C > 0 && d->C % 4 == 0 && (d->nbranch == 1 || d->nbranch == 2), "bn_train_bwd: bad geometry");
    UMR_CHECK_ARG(d->dy || (d->dpool && d->rows_per_batch > 0 && d->M % d->rows_per_batch == 0),
                  "bn_train_bwd: gradient source (dy, or dpool with rows_per_batch dividing M)");
    for (int b = 0; b < d->nbranch; ++b) {
        UMR_CHECK_ARG(d->z[b] && d->mean[b] && d->rstd[b] && d->dgamma[b] && d->dbeta[b], "bn_train_bwd: null branch pointer");
        UMR_CHECK_ARG(!apply || (d->gamma[b] && d->dz[b]), "bn_train_bwd_apply: null gamma / dz");
    }
    UMR_CHECK_ARG(apply || (d->workspace && d->workspace_bytes >= umr_bn_train_workspace(d->M, d->C)), "bn_train_bwd_reduce: workspace too small");
    a.dy = d->dy; a.dpool = d->dpool; a.y = d->y; a.g_out = d->g_out;
    for (int b = 0; b < 2; ++b) {
        const int k = b < d->nbranch ? b : 0;
        a.z[b] = d->z[k]; a.mean[b] = d->mean[k]; a.rstd[b] = d->rstd[k]; a.gamma[b] = d->gamma[k];
        a.dgamma[b] = d->dgamma[k]; a.dbeta[b] = d->dbeta[k]; a.dz[b] = d->dz[k];
    }
    a.rpb = d->rows_per_batch > 0 ? d->rows_per_batch : 1;
    a.scale = d->pool_scale; a.M = d->M; a.C = d->C; a.nb = d->nbranch;
    return UMR_OK;
}

extern "C" int umr_bn_train_bwd_reduce(const umr_bn_bwd_desc* d, umr_stream_t stream) {
    BwdArgs a;
    const int st = bwd_args(d, a, false);
    if (st != UMR_OK) return st;
    const int chunks = bn_chunks(d->M, d->C);
    const int rpc = (d->M + chunks - 1) / chunks;
    float* part = (float*)d->workspace;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(d->dtype, hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, dim3((d->C + kTileC - 1) / kTileC, chunks), dim3(256), 0, s, a, part, rpc));
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((d->C + 3) / 4), dim3(256), 0, s, a, (const float*)part, chunks);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_bn_train_bwd_apply(const umr_bn_bwd_desc* d, umr_stream_t stream) {
    BwdArgs a;
    const int st = bwd_args(d, a, true);
    if (st != UMR_OK) return st;
    const int64_t total4 = (int64_t)d->M * (d->C / 4);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(d->dtype, hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(grid_cap(total4)), dim3(256), 0, s, a));
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_maxpool3x3s2_bwd(const void* dy, const void* x, void* dx, int B, int H, int W, int C, int dtype, umr_stream_t stream) {
    UMR_CHECK_ARG(dy && x && dx, "maxpool3x3s2_bwd: null pointer");
    UMR_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "maxpool3x3s2_bwd: bad geometry");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t total = (int64_t)B * H * W * (C / 4);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel<T>, dim3(grid_cap(total)), dim3(256), 0, s, (const T*)dy, (const T*)x, (T*)dx,
                                         B, H, W, C, Ho, Wo));
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_stuff2_add(const void* src, void* dst, int B, int H, int W, int C, int dtype, umr_stream_t stream) {
    UMR_CHECK_ARG(src && dst, "stuff2_add: null pointer");
    UMR_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "stuff2_add: bad geometry");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL(stuff2_add_kernel<T>, dim3(grid_cap(total)), dim3(256), 0, s, (const T*)src, (T*)dst, B, H, W, Ho, Wo, C));
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_bce_sigmoid(const float* logit, const float* label, float* loss, float* dlogit, int B, umr_stream_t stream) {
    UMR_CHECK_ARG(logit && label && loss && dlogit, "bce_sigmoid: null pointer");
    UMR_CHECK_ARG(B > 0, "bce_sigmoid: bad geometry (B > 0)");
    hipLaunchKernelGGL(bce_sigmoid_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logit, label, loss, dlogit, B);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
