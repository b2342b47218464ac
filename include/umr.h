/* unmore_amd C-ABI: hand-written gfx950 (MI355X) kernels for unMORE's stage-1
 * ObjectnessNet hot path.  Plain pointers + extents + a HIP stream; the caller
 * (PyTorch, or any host) owns every buffer; nothing here allocates, synchronises
 * or throws.  Every entry point returns 0 on success, a negative umr_status
 * otherwise (umr_last_error_string() has the text).
 *
 * The reference (pure PyTorch, no FFI) has no C interface to mirror, so each
 * entry point cites the reference Python op(s) it replaces (paths relative to the
 * reference root).  Activations are NHWC / [rows, channels] row-major; weights
 * are passed pre-packed as documented per entry point.
 */
#ifndef UMR_H
#define UMR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* umr_stream_t; /* hipStream_t */

enum umr_status { UMR_OK = 0, UMR_ERR_INVALID = -1, UMR_ERR_UNSUPPORTED = -2, UMR_ERR_HIP = -1000 };
/* UMR_BF16X3 (umr_gemm_nt only): f32 VALUES held as three bf16 planes per value, x = h + m + l (exact for every finite f32 in
 * bf16's exponent range; written by umr_split3 or by a GEMM with UMR_EPI_OUT_X3).  A row of K logical elements is
 * [h(K) | m(K) | l(K)], 3K bf16; see umr_gemm_desc. */
enum umr_dtype { UMR_F32 = 0, UMR_BF16 = 1, UMR_BF16X3 = 2 };

int umr_version(void);
const char* umr_last_error_string(void);

/* ---- how UMR_F32 GEMMs (umr_gemm_nt / umr_gemm_tn with dtype UMR_F32; the reference computes in fp32,
 * object_reasoning.py:74) form their products.  Process-wide, may be changed between launches (not per stream).
 *   UMR_F32_EXACT: v_mfma_f32_*_f32 -- IEEE f32 multiply-adds; inf / NaN / denormal operands behave as in an f32 FMA chain.
 *   UMR_F32_X3 (default; env UMR_F32_X3=0 selects EXACT at load): every operand is split into three bf16 terms x = h + m + l
 *     and a product is six bf16 MFMAs accumulated in f32 (hh + hm + mh + hl + lh + mm; the dropped terms are <= 2^-26 of the
 *     product).  fp32-GRADE, not bit-identical to an f32 FMA chain: rms error vs float64 equals the f32 MFMA's for FINITE
 *     operands with 2^-100 < |x| < 2^126.  Outside that range it is NOT IEEE: an inf operand gives NaN (inf - inf in the split),
 *     |x| within 2^-8 of FLT_MAX rounds its leading term to inf -> NaN, and the m / l terms of |x| < 2^-110 underflow in
 *     bf16 (the product then keeps only 8 / 16 significant bits -- of a value that is itself ~1e-33).  A NaN operand gives NaN
 *     in both modes.  tests/test_gemm_gpu.py::test_f32_x3_* pins this behaviour.
 *   UMR_F32_X3_FAST (opt-in, never a default): as X3, but the UMR_BF16X3 plane GEMMs keep only the three leading terms
 *     (hh + hm + mh): every product to 2^-16 instead of 2^-24, at half the matrix work.  Meant for inference
 *     under a 1e-4 output tolerance (measured field error and peak-index agreement: bench.py --workload cfg5, alt_fp32_3term);
 *     the non-plane f32 kernels behave as in X3. */
enum umr_f32_mode { UMR_F32_EXACT = 0, UMR_F32_X3 = 1, UMR_F32_X3_FAST = 2 };
int umr_set_f32_mode(int mode);   /* returns UMR_OK or UMR_ERR_INVALID */
int umr_get_f32_mode(void);

/* CU budget of the persistent GEMM grids (umr_gemm_nt on the 256x256 kernel: one workgroup owns a CU's whole LDS).  0 (default;
 * env UMR_CU_BUDGET) = the grid is a small multiple of the CU count and the dispatcher balances it; n > 0 = the grid is exactly
 * min(n, CUs) workgroups, so the other CUs stay free for kernels that must run BESIDE it -- RCCL's all-reduce of the previous
 * gradient bucket during backward (data-parallel training, train_objectness_net.py has no such step: build-defined).  Tile shape
 * and K-split are planned on the device's CU count either way, and every output element's K sum is the same instruction
 * sequence in any workgroup: results are bit-identical across budgets.  The weight-gradient kernel (umr_gemm_tn) launches
 * (split, tile) workgroups whose count does not depend on the CU count and needs no budget.  Process-wide, run-time. */
int umr_set_cu_budget(int cus);   /* returns UMR_OK or UMR_ERR_INVALID */
int umr_get_cu_budget(void);

/* Debug / A-B options (forced tile sizes, split-K factors, kernel variants: the UMR_* names csrc/umr_common.h lists).  Process-wide.
 * The environment variable of the same name is read ONCE, when the library is loaded -- no entry point calls getenv() on its launch
 * path, so the library's behaviour never depends on environment changes made while it runs and is safe beside a host that calls
 * setenv(); tests and probes switch an option between launches with this call instead.  value: the text the environment variable
 * would hold ("256", "0", "m"), NULL = unset (the library's own default).  Unknown names return UMR_ERR_INVALID.  None of these
 * options changes WHAT is computed beyond rounding order where the option's test says so; they exist to compare forms. */
int umr_set_debug_option(const char* name, const char* value);
int umr_get_debug_option(const char* name, int* value, int* is_set);   /* letter options report the character code */

/* ---- GEMM "NT" with implicit 3x3 convolution and fused epilogue ------------
 * C[M,N] = epi(A[M,K] . B[N,K]^T), fp32 accumulate on MFMA.
 * Replaces torch.nn.Linear / 1x1 nn.Conv2d (models/dpt/vit.py:84,263-327,
 * models/dpt/blocks.py:347-355, models/objectness_net.py:110,114), timm
 * Attention.qkv/proj, Mlp.fc1/fc2, and -- with conv != 0 -- 3x3 nn.Conv2d
 * forward / data-gradient (models/dpt/blocks.py:80-115,262-280,
 * models/dpt/vit.py:329-335, models/objectness_net.py:112).
 * epilogue order: v = acc (+bias[n]) (+rowbias[m/rows_per_batch][n]);
 *   MASK_RELU: v *= (aux>0) | MASK_DGELU: v *= gelu'(aux) | ADD_AUX: v += aux;
 *   ADD_AUX2: v += aux2;  c2_mode==2: C2 = v;  v = act(v);  C = v;
 *   c2_mode==1: C2 = relu(v).
 * Rounding: fp32 (parity mode) applies every step in f32 and rounds once.  On the bf16 large-tile path the aux steps
 * (ADD_AUX, MASK_RELU, MASK_DGELU) act on the value already rounded to bf16 -- bf16(bf16(acc + bias) op aux), what separate
 * bf16 layers compute; for MASK_RELU that is bit-identical to rounding last. */
enum umr_epi_flags {
    UMR_EPI_BIAS = 1, UMR_EPI_ADD_AUX = 2, UMR_EPI_MASK_RELU = 4, UMR_EPI_MASK_DGELU = 8,
    UMR_EPI_ADD_AUX2 = 16, UMR_EPI_OUT_F32 = 32, UMR_EPI_ROWBIAS = 64,
    UMR_EPI_OUT_X3 = 128,  /* dtype UMR_BF16X3 only: C is written as three bf16 planes [h(N) | m(N) | l(N)] per row (ldc >= 3N) */
    /* dtype UMR_BF16X3 only: the operand is given as / written as bf16 planes ([M][3N], row stride >= 3N) instead of f32 [M][N] */
    UMR_EPI_AUX_X3 = 256, UMR_EPI_AUX2_X3 = 512, UMR_EPI_C2_X3 = 1024
};
enum umr_act { UMR_ACT_NONE = 0, UMR_ACT_RELU = 1, UMR_ACT_GELU = 2, UMR_ACT_TANH = 3, UMR_ACT_SIGMOID = 5 /* 4 = sine, head_out only */ };

typedef struct umr_gemm_desc {
    const void* A;        /* [M,K] rows (lda) or NHWC input when conv != 0 */
    const void* B;        /* [N,K] rows (ldb); conv: [N][3][3][Cin] */
    void* C;              /* [M,N] (ldc), dtype or f32 with UMR_EPI_OUT_F32 */
    void* C2;             /* optional second output (ldc2), dtype */
    const float* bias;    /* [N] f32 */
    const void* aux;      /* [M,N] (ldaux), dtype */
    const void* aux2;     /* [M,N] (ldaux2), dtype */
    const float* rowbias; /* [ceil(M/rows_per_batch), N] f32 */
    int64_t lda, ldb, ldc, ldc2, ldaux, ldaux2;
    int32_t M, N, K;
    int32_t dtype;        /* umr_dtype of A, B, aux, aux2, C2 (and C) */
    int32_t flags, act, c2_mode, rows_per_batch;
    int32_t conv;         /* 0 plain; 1 = 3x3 stride 1 pad 1; 2 = 3x3 stride 2 pad 1 */
    int32_t nb, H, W, Cin, Ho, Wo; /* conv geometry: A is [nb,H,W,Cin]; M = nb*Ho*Wo; K = 9*Cin */
    /* optional row remaps (0 = identity): logical row m -> (m / rows_in) * rows_out + row_off + m % rows_in.
     * a_*: rows of A (plain mode); c_*: rows of C, C2, aux, aux2 (token buffers with a class-token row per image,
     * models/dpt/vit.py:87-88,188-193).  aux_mod > 0: aux row = m % aux_mod (broadcast over images: pos-embed add, vit.py:193) */
    int32_t a_rows_in, a_rows_out, a_row_off;
    int32_t c_rows_in, c_rows_out, c_row_off;
    int32_t aux_mod;
    /* optional fused row reduction (the 1024 -> {1,2} output layer of a head, objectness_net.py:116,133, folded into the
     * epilogue of the layer that produces its input): for each 64-column slice t of the output,
     *   red_out[t][m][c] = sum_{n in slice t} C[m,n] * red_w[c][n]      (C as stored: after bias / activation / rounding)
     * red_w: [red_c][N] f32, red_c in {1,2}; red_out: [ceil(N/64)][M][red_c] f32 partial sums, summed in fixed order by
     * umr_head_out_finish.  no_store = 1 skips the store of C itself (inference: the activation is not needed again).
     * Only the persistent 256x256 bf16 path with a bias / ReLU-only epilogue implements it: call
     * umr_gemm_nt_rowreduce_ok first; umr_gemm_nt fails (UMR_ERR_UNSUPPORTED / UMR_ERR_INVALID) rather than silently
     * ignoring the request. */
    const float* red_w;
    float* red_out;
    int32_t red_c;
    int32_t no_store;
} umr_gemm_desc;

/* dtype UMR_BF16X3 -- the fast form of the fp32 parity mode (the reference runs in fp32, object_reasoning.py:74,
 * train_objectness_net.py:81): both operands are f32 values pre-split into bf16 planes; the product is the six-term sum of
 * UMR_F32_X3 (same accuracy and the same range caveats) computed as six bf16 K-tiles per logical K-tile on the persistent 256x256
 * kernel, with no split arithmetic in the loop.  A: [M][3K] bf16 (lda >= 3K; no A-row remap), or NHWC with 3*Cin bf16 per pixel
 * [h(Cin) | m(Cin) | l(Cin)] when conv == 1; B: [N][3K] bf16 (ldb >= 3K; conv: K = 9*Cin ordered (ky,kx,ci) inside each plane).
 * K (conv: Cin) must be a multiple of 64, N of 8.  Epilogue: everything umr_gemm_desc describes except tanh / sigmoid, in f32
 * (GELU = the exact erf form): bias, rowbias, one of ADD_AUX / MASK_RELU / MASK_DGELU, ADD_AUX2, c2_mode 1 / 2, act none / ReLU /
 * GELU, C-row remap and aux_mod (plain GEMM).  Operand FORMATS: C is f32 [M][N] (UMR_EPI_OUT_F32) or planes [M][3N]
 * (UMR_EPI_OUT_X3) -- exactly one of the two; aux / aux2 / C2 are f32 [M][N] unless UMR_EPI_AUX_X3 / AUX2_X3 / C2_X3 say planes
 * (a plane operand is read back as h + m + l = the f32 value; the ReLU mask reads only h, whose sign is the value's).  Or, for a
 * plain GEMM at inference, the fused row reduction red_* with no_store = 1 (bias / ReLU only; dot products of the f32 values, C
 * never stored).  Anything else returns UMR_ERR_UNSUPPORTED.
 * Small problems (the transformer at a few thousand tokens, 3x3 convs on the 4x4 ... 64x64 DPT maps: fewer tiles than CUs, or a
 * ragged last round) are cut along K into work items whose f32 partial sums go to workspace slabs, added in slab order by a
 * second launch that applies the epilogue (bitwise reproducible): pass umr_gemm_nt_ws a workspace of
 * umr_gemm_nt_workspace() + umr_gemm_nt_x3_workspace(d) bytes (the latter 0 when the problem is not split). */
int umr_gemm_nt(const umr_gemm_desc* d, umr_stream_t stream);
/* Same, with a scratch buffer that lets small problems use split-K: plain GEMMs with few 128x128 tiles and a long K (the
 * transformer's projections at a few thousand tokens -- the reference's own recipe trains on 128x128 images, batch 20 = 1300
 * tokens, README.md:148-155, train_objectness_net.py:783-788,815-817) run as tiles x splits workgroups; partial accumulators go to the workspace and the
 * workgroup that arrives last at a tile adds them in split order (bitwise reproducible) and runs the epilogue.  workspace:
 * umr_gemm_nt_workspace() bytes of device memory, 16-byte aligned, whose first 16 KiB are ZERO on first use (tile counters; every
 * launch leaves them zero) and which no other stream uses concurrently.  workspace == NULL is umr_gemm_nt. */
/* HARD PRECONDITIONS of the workspace (the split-K hand-over is a ticket counter per tile; csrc/gemm_nt.hip documents the memory
 * ordering it relies on): (1) its first 16 KiB are zero before the first launch that uses it; (2) it belongs to ONE stream -- two
 * launches that may run concurrently must not share it (results would be silently wrong); (3) a launch that was enqueued and then
 * aborted (device fault, reset) leaves counters undefined: zero them again before reuse (umr_gemm_nt_ws does so itself when the
 * launch call reports an error).  A ticket outside [0, splits) -- i.e. a violated precondition -- does NOT trap (no entry point of
 * this library aborts the process or the device context): the kernel counts it in the workspace's error word (the last of the 4096
 * counter ints), heals the counter and leaves that output tile unwritten; umr_gemm_nt_ws_status reads and clears the word.  The
 * textbook agent-scope release / acquire hand-over -- the slow reference form the default is tested against, bit for bit -- is
 * available at run time (umr_set_debug_option("UMR_SPLITK_FENCE", "1"); the environment variable of that name is read once, when the
 * library is loaded) and as a build (libumr_fence.so, make fence).  The default form's reliance on sc1 write-through
 * stores and sc1 loads is the chip's documented behaviour, not a promise of the HIP memory model: DESIGN.md section 4 quotes the guide.
 * umr_gemm_nt_splits: the number of K ranges umr_gemm_nt_ws would use for d with a workspace of that size (1 = not split). */
int64_t umr_gemm_nt_workspace(void);
int umr_gemm_nt_splits(const umr_gemm_desc* d, int64_t workspace_bytes);
int64_t umr_gemm_nt_x3_workspace(const umr_gemm_desc* d);   /* extra bytes a UMR_BF16X3 problem wants for its K-split slabs */
int umr_gemm_nt_ws(const umr_gemm_desc* d, void* workspace, int64_t workspace_bytes, umr_stream_t stream);
/* Diagnostic, and the ONE entry point that synchronises (it waits for `stream`): *bad_tickets = the number of out-of-range split-K
 * tickets seen on this workspace since the last call (0 = every split GEMM that used it wrote all of its tiles); clears the count. */
int umr_gemm_nt_ws_status(void* workspace, umr_stream_t stream, int* bad_tickets);
/* rows x K f32 (row stride ld_src elements) -> rows x [h(K) | m(K) | l(K)] bf16 (row stride ld_dst >= 3K elements):
 * h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round-to-nearest-even each.  K % 4 == 0. */
int umr_split3(const float* src, void* dst, int64_t rows, int K, int64_t ld_src, int64_t ld_dst, umr_stream_t stream);
/* the inverse: rows x [h(K) | m(K) | l(K)] bf16 -> rows x K f32, x = (h + m) + l (exact) */
int umr_unsplit3(const void* src, float* dst, int64_t rows, int K, int64_t ld_src, int64_t ld_dst, umr_stream_t stream);
/* the same with a gather of source rows: destination row r is source row (r / rows_in) * rows_out + row_off + r % rows_in (rows_in
 * == 0: identity) -- the token rows of every image without its class-token row (models/dpt/vit.py:87-88) as a compact operand */
int umr_split3_rows(const float* src, void* dst, int64_t rows, int K, int64_t ld_src, int64_t ld_dst, int rows_in, int rows_out,
                    int row_off, umr_stream_t stream);
/* 1 if umr_gemm_nt would run d (ignoring red_*, no_store) on the path that implements the fused row reduction */
int umr_gemm_nt_rowreduce_ok(const umr_gemm_desc* d);

/* ---- weight-gradient GEMM "TN" (reduction over rows) -----------------------
 * dW[N,K] (f32) = sum_m dY[m,N]^T . X[m,K]   (X rows shifted per tap when conv != 0,
 * K = 9*Cin, dW laid out [N][3][3][Cin]).  Replaces the autograd weight
 * gradients of the modules listed above (train_objectness_net.py:259).
 * Split over `splits` row ranges into workspace slabs [splits][N][K] f32, then
 * reduced in fixed order (bitwise reproducible).  workspace_bytes must be
 * >= umr_gemm_tn_workspace(d).
 * dtype UMR_BF16X3: dY [M][h(N) | m(N) | l(N)] and X [M][h(K) | m(K) | l(K)] (conv == 1: NHWC pixels of [h(Cin) | m(Cin) |
 * l(Cin)]) hold f32 values as bf16 planes (lddy >= 3N, ldx >= 3K); dW / dbias are the fp32-grade six-term products / sums (see
 * umr_gemm_nt).  N, K (conv: Cin) multiples of 8; any map size; no row remaps, no stride-2 conv (UMR_ERR_UNSUPPORTED). */
typedef struct umr_gemm_tn_desc {
    const void* dY;       /* [M,N] (lddy) */
    const void* X;        /* [M,K] (ldx) or NHWC input when conv != 0 */
    float* dW;            /* [N,K] f32 (lddw) */
    float* dbias;         /* optional [N] f32: column sums of dY */
    void* workspace;
    int64_t workspace_bytes;
    int64_t lddy, ldx, lddw;
    int32_t M, N, K;
    int32_t dtype;
    int32_t accumulate;   /* dW += instead of = */
    int32_t conv, nb, H, W, Cin, Ho, Wo;
    /* optional row remaps (0 = identity), as in umr_gemm_desc: dy_* for dY rows, x_* for X rows (plain mode) */
    int32_t dy_rows_in, dy_rows_out, dy_row_off;
    int32_t x_rows_in, x_rows_out, x_row_off;
} umr_gemm_tn_desc;

int64_t umr_gemm_tn_workspace(const umr_gemm_tn_desc* d);
int umr_gemm_tn(const umr_gemm_tn_desc* d, umr_stream_t stream);

/* ---- LayerNorm over rows of D (timm LayerNorm eps 1e-6 inside Block; vit.py:196-199) ----
 * fwd with dtype UMR_BF16X3: x is f32, y is written as bf16 planes [M][h(D) | m(D) | l(D)] (the operand of the plane GEMMs).
 * bwd: dx = LN'(dy) (+ dres if non-null: residual-branch gradient), dgamma/dbeta (f32, =/+= per `accumulate`). */
int umr_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                      int M, int D, float eps, int dtype, umr_stream_t stream);
int64_t umr_layernorm_bwd_workspace(int M, int D);
int umr_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                      const void* dres, void* dx, float* dgamma, float* dbeta, int accumulate, void* workspace,
                      int64_t workspace_bytes, int M, int D, int dtype, umr_stream_t stream);
/* The same in two steps.  _rows: dx (+ dres) and the per-workgroup partial sums of dgamma / dbeta -> workspace; _params: dgamma / dbeta
 * from those partial sums.  The second step is a weight-gradient computation: the caller may run it on the stream that carries the weight
 * gradients, behind the first, provided `workspace` is left alone until it has run (umr_layernorm_bwd = both on one stream). */
int umr_layernorm_bwd_rows(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                           const void* dres, void* dx, void* workspace, int64_t workspace_bytes, int M, int D, int dtype,
                           umr_stream_t stream);
int umr_layernorm_bwd_params(const void* workspace, int64_t workspace_bytes, float* dgamma, float* dbeta, int accumulate,
                             int M, int D, umr_stream_t stream);

/* ---- fused attention (timm Attention / F.scaled_dot_product_attention; scale head_dim^-0.5) ----
 * qkv [B*N, 3*heads*64] as produced by the qkv GEMM; out [B*N, heads*64]; lse f32 [B*heads*N].
 * bwd writes dqkv in the qkv layout; dsum_ws is scratch of umr_attention_bwd_workspace(B, N, heads) bytes
 * (per batch-head: -lse*log2(e) and rowsum(dO*O), rows padded to 64 queries). head_dim must be 64. */
int64_t umr_attention_bwd_workspace(int B, int N, int heads);
int umr_attention_fwd(const void* qkv, void* out, float* lse, int B, int N, int heads, int head_dim, int dtype,
                      umr_stream_t stream);
int umr_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* dsum_ws, void* dqkv,
                      int B, int N, int heads, int head_dim, int dtype, umr_stream_t stream);

/* ---- data movement / small ops ------------------------------------------------------------
 * patchify: NCHW f32 image -> patch rows [B*gh*gw][ldk] (K order c,py,px = Conv2d weight order; vit.py:179)
 * bilinear: NHWC resize, align_corners as given (blocks.py:155-172,377-379; vit.py:157) and its exact adjoint
 * pixel_shuffle: ConvTranspose2d with kernel == stride as GEMM + scatter (vit.py:270-302); inverse gathers
 * zero_stuff2: scatter for the data gradient of the stride-2 3x3 conv (vit.py:329-335)
 * permute4: weight packing / unpacking (4-D permutation with arbitrary, possibly negative, source strides)
 * segsum / fill_cls / cast: reductions over images, class-token row init (vit.py:188-193), dtype casts */
int umr_patchify(const float* images, void* out, int B, int H, int W, int patch, int ldk, int dtype, umr_stream_t stream);
int umr_bilinear_fwd(const void* x, void* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, int dtype, umr_stream_t stream);
int umr_bilinear_bwd(const void* dy, void* dx, int B, int Hi, int Wi, int Ho, int Wo, int C, int align_corners, int dtype, umr_stream_t stream);
/* The same resizes on maps that are column slices of wider row-major buffers: ldx / ldy (lddy / lddx) = elements between consecutive
 * pixels, 0 = C.  flags (forward): UMR_BILINEAR_RELU = max(., 0) on the result (a ReLU that follows the resize: the heads' first
 * layer runs BEFORE the final x2 interpolation of models.py:70-72 -- a 1x1 convolution and a bilinear resize commute exactly -- and
 * objectness_net.py:111's ReLU after it); UMR_BILINEAR_OUT_X3 (dtype f32, C and ldy multiples of 8) = the result as three bf16
 * planes per pixel [h(C) | m(C) | l(C)], ldy in bf16 elements (>= 3 C): the operand format of the UMR_BF16X3 GEMMs. */
#define UMR_BILINEAR_RELU 1
#define UMR_BILINEAR_OUT_X3 2
int umr_bilinear_fwd_ex(const void* x, int64_t ldx, void* y, int64_t ldy, int B, int Hi, int Wi, int Ho, int Wo, int C, int align_corners,
                        int flags, int dtype, umr_stream_t stream);
int umr_bilinear_bwd_ex(const void* dy, int64_t lddy, void* dx, int64_t lddx, int B, int Hi, int Wi, int Ho, int Wo, int C,
                        int align_corners, int dtype, umr_stream_t stream);
int umr_pixel_shuffle(const void* src, void* dst, int B, int H, int W, int s, int C, int inverse, int dtype, umr_stream_t stream);
int umr_zero_stuff2(const void* dy, void* out, int B, int H, int W, int Ho, int Wo, int C, int dtype, umr_stream_t stream);
int umr_permute4(const void* src, void* dst, const int32_t* dst_dims, const int64_t* src_strides, int64_t src_offset,
                 int dtype_in, int dtype_out, int accumulate, umr_stream_t stream);
/* many permutes in one launch (the per-step refresh of the kernel-layout weight copies after the optimizer step).
 * table_dev: n entries IN DEVICE MEMORY, sorted by blk_start; entry e covers blocks [blk_start_e, blk_start_{e+1}), blk_start_0 = 0;
 * total_blocks = the sum.  Same element semantics as umr_permute4 (dst[i0,i1,i2,i3] = src[soff + sum i_k * sstride[k]], cast to
 * dtype_out; no accumulate).  Block shape per entry: e[3] == 0 -> linear, ceil(elements / 8192) blocks of 8192 consecutive
 * destination elements; e[3] == -1 -> 2-D transpose (needs d[0] == d[1] == 1, sstride[2] == 1): ceil(d[2] / 64) * ceil(d[3] / 64)
 * blocks of 64 x 64, tile coordinate of dimension 3 fastest; otherwise TILED: a block handles the hyper-rectangle e[0] x e[1] x e[2] x e[3] (e[0] e[1] e[2] (e[3] + 1) <= 4608) of the
 * destination index space, read in source-address order (ord[] = the four dimensions by ascending |sstride|) through LDS --
 * prod_k ceil(d[k] / e[k]) blocks, tile coordinate of dimension 3 fastest.  Use tiles when the innermost destination dimension
 * is strided in the source (transposes). */
typedef struct umr_perm_entry {
    const void* src; void* dst; int32_t d[4]; int64_t sstride[4]; int64_t soff; int32_t dtype_in, dtype_out; int64_t blk_start;
    int32_t e[4]; int32_t ord[4];
    int64_t rowlen;   /* dtype_out == UMR_BF16X3: the destination is [rows][h(rowlen) | m(rowlen) | l(rowlen)] bf16 planes of the f32 values,
                         row = destination element index / rowlen (the weights of the fp32-grade plane GEMMs); otherwise ignored */
} umr_perm_entry;
/* blk_entry_dev: optional int32[total_blocks] in device memory, the entry index of every block (saves the per-block search) */
int umr_permute4_batched(const umr_perm_entry* table_dev, int n, int64_t total_blocks, const int32_t* blk_entry_dev, umr_stream_t stream);
int umr_segsum(const void* x, void* out, int R, int reps, int64_t rep_stride, int64_t seg_stride, int C, int dtype_in,
               int out_f32, int accumulate, umr_stream_t stream);
int umr_fill_cls(void* tokens, const float* cls, const float* pos0, int B, int64_t batch_stride, int D, int dtype, umr_stream_t stream);
int umr_cast(const void* src, void* dst, int64_t n, float scale, int dtype_in, int dtype_out, umr_stream_t stream);
/* dst = src * (*scalar), scalar on the device: chains the incoming gradient of the scalar loss (loss.backward(), train_objectness_net.py:259)
 * into the loss kernel's gradient maps without a host read of that scalar */
int umr_scale_by_device_scalar(const float* src, const float* scalar, float* dst, int64_t n, umr_stream_t stream);

/* ---- head output layer 1024 -> {1,2} (+tanh / sine=4), NCHW f32 output (objectness_net.py:116,133-134) ---- */
int umr_head_out_fwd(const void* h, const float* w, const float* bias, float* out, int64_t M, int K, int Cout, int HW, int act,
                     int dtype, umr_stream_t stream);
/* second half of the same layer when its dot products were folded into the producing GEMM (umr_gemm_desc.red_*):
 * out = act(bias + sum_t partials[t][m][c]), tiles added in index order (bitwise reproducible) */
int umr_head_out_finish(const float* partials, int nparts, const float* bias, float* out, int64_t M, int Cout, int HW, int act,
                        umr_stream_t stream);
int64_t umr_head_out_bwd_workspace(int64_t M, int K);
int umr_head_out_bwd(const void* h, const float* w, const float* dout, const float* yout, void* dh, float* dw, float* db,
                     void* workspace, int64_t workspace_bytes, int64_t M, int K, int Cout, int HW, int act, int relu_mask,
                     int dtype, umr_stream_t stream);

/* ---- fused 4-term loss, value + gradient (train_objectness_net.py:215-254) -----------------
 * all maps NCHW f32; out5 = [total, center, sdf, sdf-gradient, bce]; d_center / d_sdf may be NULL (value only). */
int64_t umr_loss_workspace(void);
int umr_objectness_loss(const float* pred_center, const float* pred_sdf, const float* gt_center, const float* gt_sdf,
                        const float* gt_saliency, float* d_center, float* d_sdf, float* out5, void* workspace, int B, int H,
                        int W, int center_l2, int sdf_l2, int use_grad, int use_bce, float grad_scale, umr_stream_t stream);

/* ---- Adam on a flat f32 parameter buffer (torch.optim.Adam defaults; train_objectness_net.py:96,260) ---- */
int umr_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  int step, float grad_scale, umr_stream_t stream);
/* The same update with its scalars in DEVICE memory, for a train step captured in a HIP graph and replayed with a new learning
 * rate / step count each iteration (the per-iteration MultiStepLR of train_objectness_net.py:261 changes lr between replays).
 * umr_adam_set_hyper writes hyper7 = [lr, beta1, beta2, eps, 1 - beta1^step, sqrt(1 - beta2^step), grad_scale] (one tiny launch,
 * arguments by value: no host buffer has to outlive the call); umr_adam_step_hyper is bit-identical to umr_adam_step with the
 * same arguments. */
int umr_adam_set_hyper(float* hyper7_dev, float lr, float beta1, float beta2, float eps, int step, float grad_scale, umr_stream_t stream);
int umr_adam_step_hyper(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper7_dev, umr_stream_t stream);
/* The optimizer step of a whole STAGE of the flat parameter buffer in one launch, writing the kernel-layout bf16 copies of its Linear
 * weights itself (no refresh pass that re-reads the f32 weights: -8 B per parameter and copy pair).  table_dev[i]:
 *   N == 0  a plain range: p / g / m / v of n elements, updated exactly as umr_adam_step_hyper does (4096 elements per block);
 *   N  > 0  a 2-D weight [N][K] (f32, contiguous; K % 4 == 0, N % 8 == 0, 16-byte aligned), walked in 64 x 64 tiles
 *           (ceil(N/64) * ceil(K/64) blocks, k fastest); dst_lin (may be NULL) receives bf16(p) as [N][K], dst_t (may be NULL) as [K][N].
 * blk_start = the first block of the entry, blk_entry_dev[b] = the entry of block b (int32[total_blocks]).  The update is the same
 * expression as umr_adam_step_hyper's, the copies round as umr_cast does: weights and copies are bit-identical to
 * umr_adam_step_hyper followed by umr_permute4_batched. */
typedef struct umr_adam_pack_entry {
    float* p; const float* g; float* m; float* v; void* dst_lin; void* dst_t; int64_t n; int32_t N, K; int64_t blk_start;
} umr_adam_pack_entry;
int umr_adam_pack_step(const umr_adam_pack_entry* table_dev, int n_entries, int64_t total_blocks, const int32_t* blk_entry_dev,
                       const float* hyper7_dev, umr_stream_t stream);

/* ---- object-reasoning glue around the net ("next" rows f1/f2) -----------------------
 * crop_resize: proposal crops [x1,y1,x2,y2) of a [3,H,W] f32 image -> [N,3,S,S], bilinear, no antialias
 *   (object_reasoning.py:311-323,398-410: torchvision Resize on tensors == F.interpolate(align_corners=False)).
 * center_peaks: union mask (sigmoid(sdf)>0.5 | ||center||>0.5), `erode_rounds` x (k x k) erosion, float64 5x5
 *   anti-centre correlation / 24, zero `border`, per-map max and FIRST flat argmax
 *   (object_reasoning.py:360-377,528-550; utils/misc.py:10-20).  filter50 = the 2x5x5 float64 taps (device).
 *   score_out may be NULL.  Maps up to H*W = 76,800 pixels.
 * boundary_deltas: [delta_x1, delta_y1, delta_x2, delta_y2] per map (object_reasoning.py:139-174). */
int umr_crop_resize_bilinear(const float* image, const int32_t* boxes, float* out, int N, int H, int W, int S, umr_stream_t stream);
int umr_center_peaks(const float* sdf_maps, const float* center_fields, const double* filter50, double* score_out,
                     double* max_values, int64_t* argmax, int B, int H, int W, int border, int erode_kernel, int erode_rounds,
                     umr_stream_t stream);
/* center_peaks with an argmax certificate: the same max / first flat argmax, plus certified[b] = 1 when the argmax is PROVABLY the
 * one that ANY pair of fields within `eps` (max-norm) of these would give -- the peak survives in erode(union & ~F), beats every
 * other pixel of erode(union | F) by more than 2 sqrt(2) eps (F = the pixels whose mask decision such a perturbation can flip) and
 * stays on its side of `singular_threshold` (object_reasoning.py:541); or, for a map without a positive score, no pixel of the
 * largest mask can reach one.  Lets a sweep run in a cheaper arithmetic mode and re-run only what it cannot certify
 * (unmore_amd/reasoning.py::sweep_proposals; the argument is oracle/objectness_oracle.py::peak_certificate's).  Maps up to
 * H*W = 25,600 pixels (six mask planes in LDS). */
int umr_center_peaks_certified(const float* sdf_maps, const float* center_fields, const double* filter50, double* max_values,
                               int64_t* argmax, int32_t* certified, int B, int H, int W, int border, int erode_kernel, int erode_rounds,
                               float eps, double singular_threshold, umr_stream_t stream);
int umr_boundary_deltas(const float* sdf_maps, float* deltas, int B, int H, int W, umr_stream_t stream);
/* nms: torchvision.ops.nms as object_reasoning.py:661 calls it -- `order` = the boxes' indices by descending score (the caller sorts;
 * equal scores -- the reference passes its labels, all ones -- keep their input order), greedy: a box is kept unless an earlier kept one
 * overlaps it with IoU > iou_threshold (f32: inter / (area_a + area_b - inter)).  keep[0 .. *n_keep) = the kept boxes' indices in rank
 * order; keep has room for n, n_keep is one int32 on the device.  n <= 4096; workspace: umr_nms_workspace(n) bytes, 8-byte aligned. */
/* object scoring (object_scoring.py:172-272).  Per proposal, from its S x S fields: the two binary masks (||center|| > 0.5,
 * sigmoid(sdf) > 0.5), each resized to the proposal's box (integer corners, already clipped to the image) as torchvision's Resize
 * does for integer tensors -- bilinear, align_corners=False, then round half to even -- and OR-ed (:196-228).
 * mask_paste_stats: stats[n] = {x_min, y_min, x_max + 1, y_max + 1, area} of that pasted union mask in image coordinates (the tight
 *   box of :231-235; all zero for an empty mask), maxima[n] = {max ||center||, max sdf} over the crop (:189-193).  Nothing image-sized
 *   is written.
 * mask_paste: the pasted union masks of the K selected proposals, masks [K,H,W] u8 (what survives NMS, :238-240). */
int umr_mask_paste_stats(const float* sdf_maps, const float* center_fields, const int32_t* boxes, int N, int S, int H, int W,
                         int32_t* stats, float* maxima, umr_stream_t stream);
int umr_mask_paste(const float* sdf_maps, const float* center_fields, const int32_t* boxes, const int64_t* select, int K, int S, int H, int W,
                   uint8_t* masks, umr_stream_t stream);
/* COCO run-length strings of binary masks (pycocotools' maskApi.c format; the `segmentation` of the records object_scoring.py:166-170,
 * 257-272 writes): pixels in column-major order (j = x*H + y), counts = lengths of the alternating runs starting with zeros, run i
 * written as counts[i] - (i > 2 ? counts[i-2] : 0) in 5-bit groups (low first, 0x20 = another follows, character = group + 48).
 * rle_encode: masks [K,H,W] u8 on the device (0 = clear, anything else = set).  mask_paste_rle: the pasted union masks of the K selected
 *   proposals -- the arguments and, bit for bit, the masks of umr_mask_paste -- encoded from the two crop masks in LDS over the box's
 *   columns only; the masks themselves are never written.
 * Both run as two passes over caller-owned buffers (the library allocates nothing, there is no workspace):
 *   measure: chars == NULL; sizes[k] = {number of runs, number of characters} (int64 [K][2]; the worst case is H*W + 1 runs).
 *   write:   chars != NULL; mask k's characters go to chars[offsets[k] ...) (int64 [K], the caller's prefix sum of the measured
 *            character counts; no terminator); nothing is stored at or beyond chars_capacity.  sizes is not touched.
 * The same input gives the same bytes on every run.  H*W < 2^31; rle_encode with W > 1: H <= 32764 (UMR_ERR_UNSUPPORTED beyond);
 * mask_paste_rle: S <= 256. */
int umr_rle_encode(const uint8_t* masks, int K, int H, int W, int64_t* sizes, const int64_t* offsets, uint8_t* chars, int64_t chars_capacity,
                   umr_stream_t stream);
int umr_mask_paste_rle(const float* sdf_maps, const float* center_fields, const int32_t* boxes, const int64_t* select, int K, int S, int H, int W,
                       int64_t* sizes, const int64_t* offsets, uint8_t* chars, int64_t chars_capacity, umr_stream_t stream);
/* rle_decode: the other direction, K strings -> G masks, parsed on the device (utils/preprocess_votecut.py:71-94 and
 * utils/vis_votecut.py:57-79 without pycocotools / cv2).  chars: the characters of the K strings packed in one buffer, string k =
 * chars[char_offsets[k] .. char_offsets[k+1]) (int64 [K+1], char_offsets[K] == total_chars).  Output g is a row-major [H,W] u8 mask at
 * out + out_desc[g][2] with (H, W) = out_desc[g][0..1] (int64 [G][3]; ragged: every output has its own size and byte offset), made from
 * the records group_start[g] .. group_start[g+1]-1 (int32 [G+1], ascending, group_start[0] == 0, group_start[G] == K), which all have
 * that size.  A set pixel is written as `value`, a clear one as 0; an empty group gives an all-zero mask.  max_pixels: the largest
 * H*W in out_desc (< 2^31).
 *   mode 0: the OR of the group's records.
 *   mode 1: the largest 4-connected component of the group's one record: largest area, ties to the
 *           component whose first pixel in raster order comes first (np.argmax over cv2.connectedComponentsWithStats' areas).
 *           info[g] = (number of components, area of the kept one) (int32 [G][2]; (0, 0) for an empty mask).  seg_offsets: int64 [G+1],
 *           the caller's prefix sum of nchars/2 + 1 + W per record (an upper bound of the column-split runs of ones, known without
 *           parsing); total_segments = seg_offsets[G].  mode 0 ignores seg_offsets, total_segments and info.  K != G is
 *           UMR_ERR_INVALID.  With K == G, a group_start that still gives a group two records or none is seen on the device only:
 *           every such group gets an all-zero mask and status 8 on each of its records (a group without records has none to mark:
 *           one of the others then holds two).
 * status[k] (int32 [K]): 0 = ok, else a bit set: 1 a character outside the format or a string that stops inside a number, 2 a number
 * of more than 7 characters or a count outside [0, H*W], 4 counts that do not sum to H*W, 8 a table entry out of range.  A record
 * with non-zero status is never labelled and contributes nothing (mode 1: an all-zero mask).  Nothing is stored outside
 * [out, out + out_bytes), status, info and the workspace, whatever the strings say.  The caller owns every buffer; workspace >=
 * rle_decode_workspace(K, total_chars, total_segments, mode) bytes, 8-byte aligned.  Two launches, no synchronisation; the same input
 * gives the same bytes on every run. */
int64_t umr_rle_decode_workspace(int K, int64_t total_chars, int64_t total_segments, int mode);
int umr_rle_decode(const uint8_t* chars, const int64_t* char_offsets, int K, int64_t total_chars, const int64_t* out_desc,
                   const int32_t* group_start, const int64_t* seg_offsets, int G, int64_t max_pixels, int64_t total_segments, uint8_t* out,
                   int64_t out_bytes, int value, int mode, int32_t* status, int32_t* info, void* workspace, int64_t workspace_bytes,
                   umr_stream_t stream);
/* poly_rle: the run-length records of POLYGON segmentations (pycocotools' annToRLE: maskApi.c rleFrPoly per polygon, rleMerge = union
 * over an annotation's polygons).  xy: double [n_vertices][2], the polygons' vertices one after the other; polygon q = vertices
 * poly_offsets[q] .. poly_offsets[q+1]-1 (int64 [n_polygons+1], at least one vertex each); annotation a = polygons ann_polys[a] ..
 * ann_polys[a+1]-1 (int64 [n_annotations+1]; none: an empty mask) on an image of ann_sizes[a] = (H, W) (int64 [n_annotations][2], H*W <
 * 2^31).  cross_offsets (int64 [n_polygons+1], crossing_capacity = cross_offsets[n_polygons]): the caller's prefix sum of an upper
 * bound of every polygon's column crossings -- sum over its edges of min(dx, W) + 1, dx = |x[j+1] - x[j]| with x = (int)(5*xy + .5);
 * a polygon's crossings beyond its bound are dropped, never stored elsewhere.  |xy| <= 2^20 and finite (the caller checks).
 * All double arithmetic is uncontracted IEEE in maskApi.c's operation order.  phases: a mask of 1 = the crossings, 2 = their sort,
 * 4 = the characters; 4 is the measure pass (chars == NULL) or the write pass of umr_rle_encode, over the workspace that phases 1 and
 * 2 of an earlier call on the same tables left: a caller runs 7 to measure, then 4 to write.  Every store is guarded by the record's
 * own slice and by crossing_capacity / chars_capacity.  The caller owns every buffer; workspace >= poly_rle_workspace(n_vertices,
 * n_polygons, n_annotations, crossing_capacity) bytes, 8-byte aligned.  One launch per phase, no atomics, no synchronisation; the same
 * input gives the same bytes on every run. */
int64_t umr_poly_rle_workspace(int64_t n_vertices, int n_polygons, int n_annotations, int64_t crossing_capacity);
int umr_poly_rle(const double* xy, const int64_t* poly_offsets, const int64_t* ann_polys, const int64_t* ann_sizes,
                 const int64_t* cross_offsets, int64_t n_vertices, int n_polygons, int n_annotations, int64_t crossing_capacity, int phases,
                 int64_t* sizes, const int64_t* offsets, uint8_t* chars, int64_t chars_capacity, void* workspace, int64_t workspace_bytes,
                 umr_stream_t stream);
/* COCO AP / AR evaluation (pycocotools' cocoeval.py as COCO_evaluator/coco_evaluation.py reaches it through COCOeval_opt): the two hot
 * loops, pairwise IoU and the greedy per-threshold matching.  An evaluation unit is one (image, category) pair; unit u owns the records
 * unit_start[u] .. unit_start[u+1]-1 (int32 [U+1], ascending, unit_start[0] == 0, unit_start[U] == K): first its unit_nd[u] detections,
 * in descending score order, then its ground truths.  The D_u x G_u matrices are packed row-major at pair_offsets[u] (int64 [U+1], the
 * caller's prefix sum of D_u * G_u; total_pairs = pair_offsets[U]).  crowd: uint8 [K], read for ground-truth records only.
 * mask_iou: the records are run-length strings packed as rle_decode takes them (chars, char_offsets); unit_size: int64 [U][3] =
 *   (H, W, 0), all masks of a unit share it.  inter = the integer intersection counts, area[k] = the integer area of record k, iou =
 *   (double)i / (double)(a_d + a_g - i), (double)i / (double)a_d for a crowd ground truth, 0 when that denominator is 0.  Masks are
 *   painted as bit sets over the format's column-major pixel order, 64 pixels per word, never as bytes: word_offsets (int64 [K+1]) is
 *   the caller's prefix sum of (H*W + 63) / 64 per record, total_words = word_offsets[K].  status[k] as rle_decode gives it; a record
 *   with non-zero status has area 0 and intersects nothing, the others are unaffected.  max_pixels / max_d / max_g: the largest H*W,
 *   D_u and G_u.  Workspace: mask_iou_workspace(K, total_chars, total_words) bytes, 8-byte aligned.  Three launches after the parse.
 * box_iou: boxes double [K][4] as x, y, w, h; pycocotools' bbIou in its operation order, without fused multiply-add:
 *   w = min(dx+dw, gx+gw) - max(dx, gx), 0 if w <= 0; h likewise; i = w*h; u = dw*dh + gw*gh - i (dw*dh for a crowd); i/u.
 *   max_pairs: the largest D_u * G_u.
 * coco_match: evaluateImg for every (unit, area range, threshold).  unit_nd / unit_ng: int32 [U]; det_offsets / gt_offsets: int64 [U+1]
 *   prefix sums of D_u / G_u into dt_area / gt_area (double) and gt_crowd (uint8); area_rng: double [A][2], both bounds inclusive; thr:
 *   double [T], used as passed.  A ground truth is ignored in range a when it is a crowd or its area is outside the range; per detection
 *   (the first max_det of a unit, in order) the bar starts at min(t, 1 - 1e-10); ground truths are visited non-ignored first, each
 *   group in order; one already matched and not a crowd is skipped; once a non-ignored one is held the walk stops at the first
 *   ignored one; a candidate replaces the held one when its IoU >= the bar (equal IoU: the later one); the detection inherits its
 *   match's ignore flag; an unmatched detection whose own area is outside the range is ignored.  Outputs, unit u at det_offsets[u]*A*T +
 *   ((a*T + t)*D_u + d): dt_matched (uint8), dt_gt (int32, the ground truth's index inside its unit or -1), dt_ignore (uint8);
 *   detections beyond max_det get (0, -1, 1).  gt_ignore (uint8) at gt_offsets[u]*A + a*G_u + g; gt_matched (uint8) at
 *   gt_offsets[u]*A*T + (a*T + t)*G_u + g.  A unit whose table entries point outside the buffers is left unwritten.
 * The caller owns every buffer; no synchronisation; the same input gives the same bytes on every run. */
int64_t umr_mask_iou_workspace(int K, int64_t total_chars, int64_t total_words);
int umr_mask_iou(const uint8_t* chars, const int64_t* char_offsets, int K, int64_t total_chars, const int64_t* unit_size,
                 const int32_t* unit_start, const int32_t* unit_nd, const int64_t* pair_offsets, const int64_t* word_offsets,
                 const uint8_t* crowd, int U, int64_t max_pixels, int max_d, int max_g, int64_t total_pairs, int64_t total_words,
                 int32_t* inter, double* iou, int32_t* area, int32_t* status, void* workspace, int64_t workspace_bytes,
                 umr_stream_t stream);
int umr_box_iou(const double* boxes, const int32_t* unit_start, const int32_t* unit_nd, const int64_t* pair_offsets, const uint8_t* crowd,
                int U, int K, int64_t max_pairs, int64_t total_pairs, double* iou, umr_stream_t stream);
int umr_coco_match(const double* iou, const int64_t* pair_offsets, int64_t total_pairs, const int32_t* unit_nd, const int32_t* unit_ng,
                   const int64_t* det_offsets, int64_t total_dets, const int64_t* gt_offsets, int64_t total_gts, const double* dt_area,
                   const double* gt_area, const uint8_t* gt_crowd, const double* area_rng, int A, const double* thr, int T, int max_det,
                   int U, uint8_t* dt_matched, int32_t* dt_gt, uint8_t* dt_ignore, uint8_t* gt_ignore, uint8_t* gt_matched,
                   umr_stream_t stream);
/* mask_components: 8-connected components of every map's union mask (sigmoid(sdf) > 0.5 | ||center|| > 0.5) in scipy.ndimage.label's
 * order (by first pixel in raster order) -- object_reasoning.py:206-257, the --analyze_cc branch of center_reasoning (README.md:176).
 * counts[b] = the number of components of map b; boxes[b][i] = [x1, y1, x2, y2) of component i for i < min(counts[b], max_components),
 * zeros beyond.  S * S * 8 + max_components * 16 bytes of LDS (<= 150 KiB). */
int umr_mask_components(const float* sdf_maps, const float* center_fields, int B, int S, int max_components, int32_t* counts, int32_t* boxes,
                        umr_stream_t stream);
int64_t umr_nms_workspace(int n);
int umr_nms(const float* boxes, const int64_t* order, int n, float iou_threshold, void* workspace, int64_t workspace_bytes,
            int64_t* keep, int32_t* n_keep, umr_stream_t stream);

/* ---- collapsed linear head (opt-in; SURVEY.md section 7 "the sdf head has no nonlinearity before tanh") ------
 * A head whose four convolutions have no activation between them (objectness_net.py:119-142) equals ONE 3x3 conv
 * C -> 1 plus a border-dependent bias: out(p) = act( sum_{taps t inside the image at p} (kw[t].x(p+t) + tapbias10[t])
 * + tapbias10[9] ).  x is NHWC [B,H,W,C=256]; out / dout / yout are [B,1,H,W] f32; kw is [9][C] f32.
 * bwd_data: dx (+)= sum_t kw[t] * g(p-t), g = dout*act'(yout).  bwd_weight: out = [G(9*C) | n(9) | D(1)] with
 * G[t] = sum_p g(p) x(p+t), n[t] = sum_{p: p+t inside} g(p), D = sum_p g(p): all the factored weights' gradients
 * follow from these by small matrix products (umr_small_gemm_f32).  act: UMR_ACT_NONE / UMR_ACT_TANH (4 = sine, fwd only). */
int umr_linear_head_fwd(const void* x, const float* kw, const float* tapbias10, float* out, int B, int H, int W, int C, int act,
                        int dtype, umr_stream_t stream);
int umr_linear_head_bwd_data(const float* dout, const float* yout, const float* kw, void* dx, int B, int H, int W, int C, int act,
                             int accumulate, int dtype, umr_stream_t stream);
int64_t umr_linear_head_bwd_weight_workspace(int64_t M, int C);
int umr_linear_head_bwd_weight(const void* x, const float* dout, const float* yout, float* out, void* workspace,
                               int64_t workspace_bytes, int B, int H, int W, int C, int act, int dtype, umr_stream_t stream);
/* shift9: s9[q][t] = g(q - off_t) (t < 9; zero outside the image and for 9 <= t < 16), a [B*H*W][16] map of `dtype`; nd[16] f32 =
 * n[0..8], D, zeros.  G[t] = sum_q s9[q][t] x(q) and dx(q) = sum_t s9[q][t] kw[t] are then ordinary TN / NT products -- and when x is
 * a bilinear resize of a smaller map (models.py:70-72), products on THAT map after umr_bilinear_bwd_ex of s9 (16 channels). */
int64_t umr_linear_head_shift9_workspace(int64_t M);
int umr_linear_head_shift9(const float* dout, const float* yout, void* s9, float* nd, void* workspace, int64_t workspace_bytes,
                           int B, int H, int W, int act, int dtype, umr_stream_t stream);
/* gather9 (forward mirror of shift9): with taps[q][t] = kw[t] . x(q) given as a [B*H*W] map of >= 9 f32 channels (pixel stride ldt) --
 * for x = resize(y) that is the resize of the 16-column product y kw^T taken on the small map --
 * out(q) = act( sum_{t: q + off_t inside the image} (taps[q + off_t][t] + tapbias10[t]) + tapbias10[9] ), out [B,1,H,W] f32. */
int umr_linear_head_gather9(const float* taps, int64_t ldt, const float* tapbias10, float* out, int B, int H, int W, int act,
                            umr_stream_t stream);
/* C[i*sc_m + j*sc_n] (=|+=) sum_k A[i*sa_m + k*sa_k] * B[k*sb_k + j*sb_n]  (tiny f32 products, arbitrary strides) */
int umr_small_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int64_t sa_m, int64_t sa_k, int64_t sb_k,
                       int64_t sb_n, int64_t sc_m, int64_t sc_n, int accumulate, umr_stream_t stream);

/* ---- existence classifier: torchvision ResNet-50 + Linear(1000,1) + sigmoid in eval mode
 * (models/objectness_net.py:205-223; callers object_reasoning.py:491-523, object_scoring.py:123-140).  Convolutions and
 * Linear layers run on umr_gemm_nt; these are the remaining pieces.
 * im2col_nchw: NCHW f32 image -> rows [B*Ho*Wo][ldk], K order (c, ky, kx) (= Conv2d weight order), tail zero: the 7x7 s2 p3 stem
 * maxpool3x3s2: nn.MaxPool2d(kernel 3, stride 2, padding 1), NHWC
 * bn_fold: eval-mode BatchNorm2d folded into the preceding conv's packed weight rows: w_out[co][k] = w[co][k]*s, b_out[co] =
 *          beta - mean*s, s = gamma / sqrt(var + eps) */
int umr_im2col_nchw(const float* images, void* out, int B, int C, int H, int W, int KH, int KW, int stride, int pad, int ldk,
                    int dtype, umr_stream_t stream);
int umr_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, int dtype, umr_stream_t stream);
int umr_bn_fold(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, void* w_out,
                float* b_out, int Co, int K, int ldk, int dtype, umr_stream_t stream);

/* ---- existence-classifier training (train_objectness_net.py:540-743, BinaryClassifierTrainer; csrc/clf_train.hip) ----
 * Layout NHWC: a map is [M rows][C channels] with M = B*H*W; storage f32 or bf16 (dtype), statistics and sums in f32.  Every
 * reduction is deterministic: fixed row chunks per (M, C), per-chunk partials combined in a fixed order, no float atomics.
 * bn_train_stats: training-mode BatchNorm2d statistics of a raw conv output z: mean, rstd = 1/sqrt(var_biased + eps) (f32 [C]),
 *   from shifted sums (shift = row 0 of each channel; no E[x^2]-E[x]^2 cancellation).  Non-null running_mean / running_var are
 *   updated as nn.BatchNorm2d does (r = (1-momentum) r + momentum s, with the unbiased variance; M > 1), and a non-null
 *   num_batches_tracked is incremented by one.  workspace >= umr_bn_train_workspace(M, C).
 * bn_train_apply: y = act(gamma (z - mean) rstd + beta [+ gamma2 (z2 - mean2) rstd2 + beta2 | + residual]); act: 0 none, 1 ReLU.
 * bn_train_bwd_reduce / _apply (one umr_bn_bwd_desc for both): g = dy, or dpool[row / rows_per_batch] * pool_scale (the avg-pool
 *   backward, broadcast here), zeroed where the saved post-activation y <= 0 when y is given.  For each of nbranch (1 or 2) BNs
 *   that fed the same sum: _reduce writes dbeta = sum g and dgamma = sum g * xhat (xhat recomputed from z, mean, rstd);
 *   _apply reads them back and writes dz = gamma rstd (g - dbeta/M - xhat dgamma/M), and g itself to g_out when non-null.
 * maxpool3x3s2_bwd: gradient of umr_maxpool3x3s2 in gather form: each input pixel sums the gradients of the (<= 4) windows
 *   whose first maximum in (ky, kx) scan order it is, recomputed from the saved pool input x.
 * stuff2_add: dst[b][2y][2x][c] += src[b][y][x][c] (the data gradient of a stride-2 1x1 convolution scattered into the map).
 * bce_sigmoid: loss[0] = mean_i BCE(sigmoid(logit_i), label_i) with torch's clamps (log >= -100; the backward divides by
 *   max(p (1-p), 1e-12)), dlogit[i] = d loss / d logit_i; one launch. */
typedef struct umr_bn_bwd_desc {
    const void* dy;              /* [M, C] or NULL (then dpool) */
    const float* dpool;          /* [M / rows_per_batch, C] f32 */
    const void* y;               /* optional [M, C]: ReLU mask source */
    const void* z[2];            /* [M, C] raw conv outputs */
    const float* mean[2];
    const float* rstd[2];
    const float* gamma[2];
    float* dgamma[2];
    float* dbeta[2];
    void* dz[2];                 /* [M, C] (_apply) */
    void* g_out;                 /* optional [M, C] (_apply) */
    void* workspace;             /* >= umr_bn_train_workspace(M, C) bytes (_reduce) */
    int64_t workspace_bytes;
    int64_t rows_per_batch;
    float pool_scale;
    int32_t M, C, nbranch, dtype;
} umr_bn_bwd_desc;
int64_t umr_bn_train_workspace(int M, int C);
int umr_bn_train_stats(const void* z, float* mean, float* rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                       void* workspace, int64_t workspace_bytes, int M, int C, float eps, float momentum, int dtype, umr_stream_t stream);
int umr_bn_train_apply(const void* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* z2,
                       const float* mean2, const float* rstd2, const float* gamma2, const float* beta2, const void* residual, void* y,
                       int M, int C, int act, int dtype, umr_stream_t stream);
int umr_bn_train_bwd_reduce(const umr_bn_bwd_desc* d, umr_stream_t stream);
int umr_bn_train_bwd_apply(const umr_bn_bwd_desc* d, umr_stream_t stream);
int umr_maxpool3x3s2_bwd(const void* dy, const void* x, void* dx, int B, int H, int W, int C, int dtype, umr_stream_t stream);
int umr_stuff2_add(const void* src, void* dst, int B, int H, int W, int C, int dtype, umr_stream_t stream);
int umr_bce_sigmoid(const float* logit, const float* label, float* loss, float* dlogit, int B, umr_stream_t stream);

/* ---- ground-truth synthesis on the device (datasets.py:158-159,171-222 without random crop) -------
 * mask [B,H,W] u8 (non-zero = object) at the training resolution; center_xy [B,2] f32 (x, y) object centres in the same
 * pixel coordinates, or NULL = bounding-box centre of each mask ((min+max)/2, datasets.py:158-159).
 * sdf = DT(mask)/max - DT(1-mask)/max (second term only with use_bg_sdf) where DT is cv2.distanceTransform(u8, DIST_L2, 3)
 * (OpenCV's 3x3 chamfer in 16.16 fixed point, a = 0.955, b = 1.3693); center_field [B,2,H,W] = normalize(mask *
 * normalize((i - c_y, j - c_x))); saliency = mask > 0.  Empty masks give all-zero labels (datasets.py:128-138). */
int64_t umr_label_synthesis_workspace(int B, int H, int W);
int umr_label_synthesis(const uint8_t* mask, const float* center_xy, float* center_field, float* saliency, float* sdf,
                        void* workspace, int64_t workspace_bytes, int B, int H, int W, int use_bg_sdf, umr_stream_t stream);

/* ---- the random-crop branch of the training item (datasets.py:144-145,161-190: the default training path, :109) ----
 * crop_resize_batch: src [B,C,H,W] with one box [x1,y1,x2,y2) per item -> dst [B,C,Ho,Wo]; f32 bilinear (torchvision tensor
 *   Resize without antialias == F.interpolate(align_corners=False), :99,103) or, with nearest_u8, u8 nearest
 *   (F.interpolate(mode="nearest"), :100,104).  Serves transforms.Resize (box = whole image) and crop + Resize.
 * distance_transform: cv2.distanceTransform(u8, DIST_L2, 3) of each mask, divided by its maximum when normalize (:162-163).
 * label_synthesis_cropped: as label_synthesis, but the foreground field was computed before the crop and arrives resized
 *   (fg_sdf [B,H,W]), the object centres are given, only the background transform is taken from `mask`, and an empty
 *   mask is not short-circuited (the reference tests emptiness before the crop, :146-157). */
int umr_crop_resize_batch(const void* src, const int32_t* boxes, void* dst, int B, int C, int H, int W, int Ho, int Wo,
                          int nearest_u8, umr_stream_t stream);
int64_t umr_distance_transform_workspace(int B, int H, int W);
int umr_distance_transform(const uint8_t* mask, float* out, void* workspace, int64_t workspace_bytes, int B, int H, int W,
                           int normalize, umr_stream_t stream);
int umr_label_synthesis_cropped(const uint8_t* mask, const float* center_xy, const float* fg_sdf, float* center_field,
                                float* saliency, float* sdf, void* workspace, int64_t workspace_bytes, int B, int H, int W,
                                int use_bg_sdf, umr_stream_t stream);

/* ---- the existence classifier's training item (datasets.py:285-349 after file decoding) ---------------------------------
 * Items of a batch differ in size: both entry points take a RAGGED batch, a device table of B umr_ragged_src entries the
 * host uploads in one copy, and launch once for the whole batch.
 * bg_square (background branch, :304-313): per item, on its mask `u8` [H,W] (non-zero = object), the 3x3 chamfer transform
 *   of `mask == 0` with a ZERO border (what the reference's ten rings of zero padding amount to: the image edge is an
 *   obstacle), the first maximum in raster order of the float32 field (fixed * 2^-16 rounded to float32, ties decided after
 *   the conversion), r = that maximum, and the box x1 = int(x - r), y1 = int(y - r), x2 = int(x + r), y2 = int(y + r)
 *   (float64 arithmetic, truncation toward zero, clamped to the image as the slice :316 clamps).  out: int32 [B,5] =
 *   (x1, y1, x2, y2, ok), ok = 0 for an empty box (x2 <= x1 or y2 <= y1: the reference's resize raises and the item falls
 *   through to the foreground branch, :324-325).  An entry that breaks the limits below on the device comes back as
 *   (-1,-1,-1,-1,0).  max_w / max_pixels: the widest row and the largest H*W in the table (max_w > 4096: UMR_ERR_UNSUPPORTED);
 *   workspace >= bg_square_workspace(B, max_pixels): one int32 field per item, written and read once.
 * crop_resize_ragged (:316-319 and :335-346): per item the box [x1,y1,x2,y2) of its `f32` source [C,H,W] -> dst [B,C,Ho,Wo],
 *   crop_resize_batch's bilinear arithmetic.  With mask_sum != NULL one more channel: `u8` [H,W] read as u8 / 255 in f32
 *   (to_tensor) before interpolation -> mask_out [B,Ho,Wo], and its sum over the Ho*Wo resized values -> mask_sum [B] (the
 *   label is mask_sum > 1, :343).  An entry with u8 == NULL (a background-branch item) gets a zero mask and sum 0.  One
 *   workgroup per (item, channel plane); the sum adds fixed per-thread strides, then a fixed tree: bitwise reproducible,
 *   no atomics.  Boxes are clamped to the source; an empty box yields zeros. */
typedef struct umr_ragged_src {
    const float* f32;     /* [C,H,W] f32 planes (crop_resize_ragged) */
    const uint8_t* u8;    /* [H,W] u8 mask (bg_square; crop_resize_ragged: optional extra channel) */
    int32_t H, W;
} umr_ragged_src;
int64_t umr_bg_square_workspace(int B, int64_t max_pixels);
int umr_bg_square(const umr_ragged_src* items, int32_t* out, void* workspace, int64_t workspace_bytes, int B, int max_w,
                  int64_t max_pixels, umr_stream_t stream);
int umr_crop_resize_ragged(const umr_ragged_src* items, const int32_t* boxes, float* dst, float* mask_out, float* mask_sum,
                           int B, int C, int Ho, int Wo, umr_stream_t stream);

/* ---- copy-paste augmentation of the detector's training batches (cad/engine/train_loop.py:90-248, called from run_step :261-263;
 * csrc/copy_paste.hip) -----------------------------------------------------------------------------------------------------
 * A RAGGED batch of P independent pairs, one device table entry each, one sequence of launches for all of them.  Per pair: the nc
 * chosen masks choice[choice_off .. choice_off + nc) (indices into the labeled item's Nl masks) and the labeled image are resized to
 * h_new x w_new (F.interpolate, bilinear, align_corners=False: src = fmaf(r, dst + 0.5, -0.5) clamped at 0 with r = rh / rw, the float32
 * quotients in / out formed by the caller; a mask pixel is set iff a tap with a non-zero weight is set, an image byte is the float32
 * value truncated) and pasted at (h_shift, w_shift) into the unlabeled frame.  Copied instance i is kept iff for every existing
 * mask j: area_j > 0 and 2 * inter_ij < area_j (the reference's float32 inter / area < 0.5, max over j, NaN from an empty existing mask
 * included; exact for Hu * Wu < 2^24, larger frames are refused); with Nu == 0 every copy is kept.  alpha = the union of the kept
 * pasted masks; out_image [3,Hu,Wu] = alpha ? resized labeled : unlabeled; out_masks [Nu + nc,Hu,Wu] u8 (0 / 1) = the existing masks
 * & ~alpha, then the kept pasted masks (rows of copies that are not kept are left unwritten).  A pair that keeps no copy writes
 * neither: its result is the unlabeled item.  Masks are read as u8, non-zero = set.
 * stats: int32 [total_rows][2], boxes: float [total_rows][4]; the pair's rows are row_off .. row_off + Nu + nc - 1, existing first.
 *   stats[r] = (flag, area): a copied row's flag = kept; an existing row's flag = the pair keeps at least one copy.  area and box are
 *   written for rows with a non-zero flag: the area of the output mask, and its box by Detectron2's BitMasks.get_bounding_boxes rule
 *   [x_min, y_min, x_max + 1, y_max + 1] (zeros for an empty mask) when Nu > 0; with Nu == 0 the reference's own float32 box: the chosen
 *   box of l_boxes ([Nl,4] XYXY) times (sx, sy), then x0, x1 += h_shift and y0, y1 += w_shift -- the reference swaps the two shifts
 *   (:191-194) and so does this.  The caller zeroes stats before the call.
 * word_off / inter_off: the pair's slices of the workspace's two regions, (nc + Nu + 1) * Hu * ceil(Wu / 64) 64-bit words (the bit
 *   sets of the pasted masks, the existing masks and alpha) and (nc + 1) * Nu int32 (intersections, existing areas); total_words /
 *   total_inter = the regions' sizes, workspace >= copy_paste_workspace(total_words, total_inter) bytes, 8-byte aligned.
 *   max_words_per_mask, max_nc, max_nu: the largest Hu * ceil(Wu / 64), nc and Nu in the table (grid sizes only).
 * phases: a mask of 1 = pack (resize, paste, bit sets), 2 = overlap + keep decision, 4 = compose + areas and boxes; a caller that
 *   times the parts runs 1, 2, 4 one after the other on the same buffers, everyone else passes 7.
 * An entry that breaks its own bounds (sizes, shifts, slices past the totals, nc > Nl) is skipped on the device: nothing of it is read
 * or written; a choice outside [0, Nl) pastes an empty mask.  No atomics, no synchronisation, nothing allocated; the same input
 * gives the same bytes on every run. */
typedef struct umr_cp_pair {
    const uint8_t* l_image;   /* [3,Hl,Wl] u8 */
    const uint8_t* l_masks;   /* [Nl,Hl,Wl] u8 / bool */
    const float* l_boxes;     /* [Nl,4] f32 (read when Nu == 0) */
    const uint8_t* u_image;   /* [3,Hu,Wu] u8 */
    const uint8_t* u_masks;   /* [Nu,Hu,Wu] u8 / bool; may be NULL when Nu == 0 */
    uint8_t* out_image;       /* [3,Hu,Wu] u8 */
    uint8_t* out_masks;       /* [Nu + nc,Hu,Wu] u8 */
    int64_t word_off, inter_off, row_off, choice_off;
    int32_t Hl, Wl, Nl, Hu, Wu, Nu, nc, h_new, w_new, h_shift, w_shift;
    float rh, rw;             /* (float)Hl / (float)h_new, (float)Wl / (float)w_new */
    float sx, sy;             /* box scale: Wu / Wl * ratio, Hu / Hl * ratio, rounded to float32 */
    int32_t reserved;
} umr_cp_pair;
int64_t umr_copy_paste_workspace(int64_t total_words, int64_t total_inter);
int umr_copy_paste(const umr_cp_pair* pairs, int P, const int32_t* choice, int64_t total_choice, int64_t total_words,
                   int64_t total_inter, int64_t total_rows, int64_t max_words_per_mask, int max_nc, int max_nu, int phases,
                   int32_t* stats, float* boxes, void* workspace, int64_t workspace_bytes, umr_stream_t stream);

/* ---- mask-head targets and the score-weighted mask loss of the detector (cad/modeling/roi_heads/roi_heads.py:963-1045,
 * mask_rcnn_loss_weighted, "soft targets"; csrc/mask_loss.hip) -----------------------------------------------------------------------
 * R proposals in image order over a table of n_images entries; proposal r belongs to the last entry with first <= r and is its
 * proposal j = r - first: box boxes[j] (XYXY), mask index[j] (int32, or int64 with index64 != 0; NULL = the identity j) of the entry's G
 * masks -- the reference gathers one full frame per proposal first (gt_masks[matched_idxs]), here the kernel reads the mask in place.
 * Target [M,M] of a proposal: Detectron2's BitMasks.crop_and_resize = torchvision roi_align(spatial_scale 1, sampling_ratio 0,
 * aligned) of the 0 / 1 mask (non-zero byte = 1), then >= 0.5, in float32 and in torchvision's operation order (csrc/mask_loss.hip
 * writes it out).  A box that is empty (x2 <= x1 or y2 <= y1) has no samples and a zero target.
 * mask_targets: targets u8 [R,M,M] (0 / 1) only.
 * mask_loss: logits [R,C,M,M] (UMR_F32 / UMR_BF16, contiguous); the logit x of proposal r is channel 0 (C == 1) or gt_classes[r];
 *   loss[0] = mean over R*M*M of weights[r] * ((1 - t) * x + max(-x, 0) + log1p(exp(-|x|))) as float32 (terms in float32, sums in
 *   double; weights == NULL: ones; R == 0: 0); grad [R,C,M,M] in the logits' type = weights[r] * (sigmoid(x) - t) / (R*M*M) in that
 *   channel, 0 in the others; counts int64 [5] = elements with (x > 0) != t, with t, with both (x > 0) and !t, with !(x > 0) and t,
 *   and the number of BAD proposals; targets: optional u8 [R,M,M].
 * A bad proposal -- mask index outside [0, G), a box coordinate that is not finite or beyond +-2^20 -- gets a zero target and is
 *   counted; nothing of it is read out of bounds.  A class outside [0, C) is counted too and adds no loss, no count and no gradient.
 * max_h, max_w: the largest H and W in the table; they size the kernel's LDS tables, 16 * (max_h + max_w) + 32 * M + 328 bytes, at
 *   most 160 KiB (else UMR_ERR_INVALID); 1 <= M <= 512.  Work per proposal is at most (2 * (H + 4) + M) * (2 * (W + 4) + M) samples
 *   whatever its box; a proposal of more than 65536 samples is shared by ceil(M * M / 256) workgroups, whole rows of bins each.
 *   workspace >= mask_loss_workspace(R, M) bytes (one 32-byte partial per workgroup; -1 for a negative R or an M outside [1, 512]),
 *   8-byte aligned.
 * phases: a mask of 1 = targets, loss terms, gradient and the partials, 2 = the finishing sum; a caller that times the parts
 *   runs 1, 2 on the same buffers, everyone else passes 3.  No atomics, no synchronisation, nothing allocated; the same input gives
 *   the same bytes on every run. */
typedef struct umr_ml_image {
    const uint8_t* masks;     /* [G,H,W] u8 / bool */
    const float* boxes;       /* [R_i,4] f32 XYXY */
    const void* index;        /* [R_i] int32 / int64, or NULL */
    int32_t H, W, G;
    int32_t first;            /* the image's first proposal: the sum of the R_i before it */
    int32_t R;                /* R_i */
    int32_t index64;
} umr_ml_image;
int64_t umr_mask_loss_workspace(int64_t R, int M);
int umr_mask_targets(const umr_ml_image* images, int n_images, int64_t R, int M, int max_h, int max_w, uint8_t* targets,
                     umr_stream_t stream);
int umr_mask_loss(const umr_ml_image* images, int n_images, int64_t R, int C, int M, int max_h, int max_w, const void* logits,
                  int dtype, const int64_t* gt_classes, const float* weights, int phases, uint8_t* targets, void* grad,
                  float* loss, int64_t* counts, void* workspace, int64_t workspace_bytes, umr_stream_t stream);

/* ---- the box branch of the detector's cascade ROI heads (cad/modeling/roi_heads/custom_cascade_rcnn.py:166-357, fast_rcnn.py:94-121,
 * 329-390, 462-514, 574-598, cad/structures/boxes.py, cad/modeling/box_regression.py; csrc/box_loss.hip) ---------------------------------
 * R proposals in image order over a table of n_images entries, cut into chunks of 256 rows per image: entry k owns the chunks
 * [chunk_first, chunk_first + ceil(R_k / 256)) and n_chunks is their total.  Boxes are float32 XYXY.  What gt_* point to depends on the
 * entry point: box_match reads the image's G ground truths ([G,4], [G], [G]); box_loss and box_drop_weights read the MATCHED fields,
 * one row per proposal ([R_k,4], [R_k], [R_k]; box_drop_weights reads gt_boxes only); box_decode reads boxes, height and width only.
 * IoU is Detectron2's pairwise_iou in float32, every operation rounded on its own and the division correctly rounded.
 * box_match (Matcher([t], [0, 1], allow_low_quality_matches=False)): per row matched_vals = the maximum IoU over the image's ground truths,
 *   matched_idxs = the lowest index that attains it, label = matched_vals >= t; gt_classes = the matched class or num_classes, gt_boxes /
 *   gt_scores gathered by matched_idxs on every row.  G == 0: index 0, value 0, background, zero box and score.  A proposal with a
 *   non-finite coordinate is bad: index 0, value 0, background.  A NaN IoU caused by a ground truth never wins the maximum (torch's max
 *   would hand it on); a row whose every IoU is NaN is background with index 0 and value 0, and is not counted.  counts int32 [3, n_images], ZEROED BY THE CALLER: foreground,
 *   background and bad rows per image (integer atomics, one per workgroup).
 * box_decode: Box2BoxTransform.apply_deltas(deltas, boxes) with weights (wx, wy, ww, wh), Boxes.clip to (height, width) and, when
 *   training != 0, the rows with width > 0 and height > 0 only: boxes [R,4] compacted in order, image after image (tail undefined),
 *   keep u8 [R], counts int32 [n_images].  workspace >= box_decode_workspace(R, n_chunks) bytes, 4-byte aligned.
 * box_apply_deltas / box_get_deltas: the two transforms as element-wise ops over n rows.
 * box_drop_weights: weights [R] of the reference's drop-loss block: the ground-truth set of image k is the first n_k rows of its matched
 *   gt_boxes, n_k = the number of distinct rows among the first min(100, R_k); weight = !(max IoU of the row's decoded, unclipped
 *   prediction with that set <= iou_thresh); then row r takes 1 where is_single_object[r / (R / n_images)] == 1 (float32
 *   [n_images] or NULL; by POSITION, as the reference indexes it).
 * box_loss (FastRCNNOutputLayers.losses): scores [R,K1], deltas [R,4] (UMR_F32 / UMR_BF16), K1 == num_classes + 1.  drop_mode 0: weights
 *   of one, 1: weights_in [R], 2: the rule above.  loss_cls[0] = mean over R of w_r * CE_r, CE against the soft targets (fg, 1 - fg), fg =
 *   gt_scores or 0 on background rows (soft_targets != 0, K1 == 2), or against gt_classes; loss_box_reg[0] = sum over the rows with
 *   0 <= class < num_classes of smooth_l1(deltas - get_deltas(box, gt_box), beta) (* gt_scores with soft targets) / max(R, 1); terms in
 *   float32, sums in double.  grad_scores = w (softmax - target) / R and grad_deltas = smooth_l1' * score / R in the inputs' type;
 *   weights [R] = the weights used; counters int64 [7] = rows, foreground rows, argmax == class, foreground with argmax == class,
 *   foreground predicted background, rows of weight 0, bad rows (a foreground row whose proposal or ground-truth extent is not positive
 *   or finite: no box term; a class no column stands for without soft targets: no term at all).
 *   workspace >= box_loss_workspace(n_chunks) bytes (one 48-byte partial per workgroup), 8-byte aligned.  phases as in mask_loss.
 * No float atomics, no synchronisation, nothing allocated; the same input gives the same bytes on every run. */
typedef struct umr_bl_image {
    const float* boxes;          /* [R_k,4] proposals */
    const float* gt_boxes;
    const int64_t* gt_classes;
    const float* gt_scores;
    int32_t first;               /* the image's first proposal: the sum of the R before it */
    int32_t R, G;
    int32_t chunk_first;         /* the image's first chunk: the sum of ceil(R / 256) before it */
    float height, width;         /* the frame, for the clip */
} umr_bl_image;
int64_t umr_box_loss_workspace(int64_t n_chunks);
int64_t umr_box_decode_workspace(int64_t R, int64_t n_chunks);
int umr_box_match(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, float iou_threshold, int64_t num_classes,
                  int64_t* matched_idxs, float* matched_vals, int64_t* gt_classes, float* gt_boxes, float* gt_scores, int32_t* counts,
                  umr_stream_t stream);
int umr_box_decode(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, const void* deltas, int dtype, float wx, float wy,
                   float ww, float wh, int training, float* boxes, uint8_t* keep, int32_t* counts, void* workspace,
                   int64_t workspace_bytes, umr_stream_t stream);
int umr_box_apply_deltas(const void* deltas, int dtype, const float* boxes, int64_t n, float wx, float wy, float ww, float wh, float* out,
                         umr_stream_t stream);
int umr_box_get_deltas(const float* src, const float* target, int64_t n, float wx, float wy, float ww, float wh, float* out,
                       umr_stream_t stream);
int umr_box_drop_weights(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, const void* deltas, int dtype, float wx,
                         float wy, float ww, float wh, float iou_thresh, const float* is_single_object, float* weights,
                         umr_stream_t stream);
int umr_box_loss(const umr_bl_image* images, int n_images, int64_t R, int64_t n_chunks, int K1, int64_t num_classes, const void* scores,
                 const void* deltas, int dtype, float wx, float wy, float ww, float wh, float smooth_l1_beta, int soft_targets,
                 int drop_mode, float iou_thresh, const float* weights_in, const float* is_single_object, int phases, float* weights,
                 void* grad_scores, void* grad_deltas, float* loss_cls, float* loss_box_reg, int64_t* counters, void* workspace,
                 int64_t workspace_bytes, umr_stream_t stream);

/* ---- the detector's inference tail (cad/modeling/roi_heads/fast_rcnn.py:52-179, roi_heads.py:1048-1091, meta_arch/rcnn.py:242-256 with
 * Detectron2's detector_postprocess, cad/evaluation/coco_evaluation.py:398-457; csrc/det_post.hip) ----------------------------------------
 * det_select (fast_rcnn_inference for a batch): per image scores [R,K+1] (background last) and boxes [R,4] (box_classes == 1) or [R,K*4]
 *   (box_classes == K), float32.  A row with a non-finite box or score entry is dropped; boxes are clipped to (height, width); the
 *   candidates are the pairs p = r * K + c with score[r,c] > score_thresh, in p order; they are ranked by descending score, equal scores
 *   in p order; greedy NMS per class: a candidate is suppressed iff an earlier kept one of its class has
 *   inter / ((area_a + area_b) - inter) > nms_thresh (float32, every operation rounded on its own; NaN suppresses nothing); the first
 *   topk kept ones (all when topk < 0) of image k go, in rank order, to the rows [out_first, out_first + counts[k]) of out_boxes [total_out,4],
 *   out_scores, out_classes and out_rows (the input row).  Table: cand_first = the sum of R * K before the image, total_cand their
 *   total, max_cand their maximum (<= 8192); cap = the image's output slots (R * K, or min(R * K, topk)), out_first / total_out their
 *   prefix sums; mat_first = the sum of R * K * ceil(R * K / 64) before the image (64-bit words of its suppression matrix), total_words
 *   their total.  workspace >= det_select_workspace(n_images, total_cand, total_words) bytes, 16-byte aligned.  phases: 1 = candidates
 *   and ranks, 2 = the suppression matrix, 4 = the scan; 7 = all (three launches).  Nothing is read back; no atomics.
 * det_scale: rec [n,8] = the box scaled by rowinfo's (sx, sy) and clipped to its (H, W) as x0, y0, x1, y1, then x1 - x0, y1 - y0,
 *   1 / 0 for width > 0 and height > 0, and 0.  rowinfo [n,4] 32-bit words: float sx, float sy, int32 H, int32 W.
 * det_paste (paste_masks_in_image): logits [N,C,M,M] UMR_F32 / UMR_BF16, channel classes[k] when C > 1 (NULL allowed for C == 1);
 *   sigmoid, then F.grid_sample(align_corners=False, zero padding) into box k (boxes + k * box_stride floats), set iff the sample
 *   >= threshold (in [0.5, 1]); out u8 [N,H,W], ZEROED BY THE CALLER.  The float32 operation order is written out in csrc/det_post.hip.  M <= 128.
 * det_paste_rle: the COCO run-length strings of those masks without writing them, mask k in its own frame (frames + k * frame_stride:
 *   int32 H, W); the measure pass / write pass protocol of umr_rle_encode. */
typedef struct umr_dp_image {
    const float* boxes;          /* [R,4] or [R,K*4] */
    const float* scores;         /* [R,K+1] */
    int64_t mat_first;
    int32_t R;
    int32_t cand_first;
    int32_t out_first;
    int32_t cap;
    float height, width;         /* the frame, for the clip */
} umr_dp_image;
int64_t umr_det_select_workspace(int n_images, int64_t total_cand, int64_t total_words);
int umr_det_select(const umr_dp_image* images, int n_images, int K, int box_classes, int64_t total_cand, int max_cand, int64_t total_words,
                   int64_t total_out, float score_thresh, float nms_thresh, int topk, int phases, float* out_boxes, float* out_scores,
                   int64_t* out_classes, int64_t* out_rows, int32_t* counts, void* workspace, int64_t workspace_bytes,
                   umr_stream_t stream);
int umr_det_scale(const float* boxes, const void* rowinfo, int64_t n, float* rec, umr_stream_t stream);
int umr_det_paste(const void* logits, int dtype, int64_t N, int C, int M, const int64_t* classes, const float* boxes, int box_stride, int H,
                  int W, float threshold, uint8_t* out, umr_stream_t stream);
int umr_det_paste_rle(const void* logits, int dtype, int64_t N, int C, int M, const int64_t* classes, const float* boxes, int box_stride,
                      const int32_t* frames, int frame_stride, float threshold, int64_t* sizes, const int64_t* offsets, uint8_t* chars,
                      int64_t chars_capacity, umr_stream_t stream);

/* ---- the ROI pooler of the detector's heads (Detectron2's modeling/poolers.py ROIPooler with ROIAlignV2 = torchvision's
 * roi_align(aligned=True); built at cad/modeling/roi_heads/custom_cascade_rcnn.py:117-122 and roi_heads.py:674-679, 709-716;
 * csrc/roi_pool.hip) ---------------------------------------------------------------------------------------------------------------------
 * R boxes, float32 XYXY in frame coordinates: rows of box_stride 4 ([R,4], in image order, with first int32 [N + 1] = the prefix sums of
 * the boxes per image) or of box_stride 5 ([R,5] = image index as a float, then the box; first == NULL).  info int32 [R,2] = (image,
 * level) per box, (-1, 0) for a box the device refuses: an image index outside [0, N) or not an integer, a coordinate that is not finite
 * or beyond +-2^20.
 * roi_pool_prepare writes info.  n_levels > 1: Detectron2's assign_boxes_to_levels in float32, operation by operation --
 *   floor(canonical_level + log2(sqrt((x2 - x1) * (y2 - y1)) / canonical_box_size + 1e-8f)) clamped to [min_level, max_level], minus
 *   min_level; a NaN (a negative area) gives level 0.  n_levels == 1: level 0.
 * levels: a HOST array of 4 int64 per level, at most 8 levels, copied into the kernel's arguments by value (nothing is uploaded):
 *   the pointer of the level's map [N,C,H,W] (UMR_F32 / UMR_BF16, contiguous), H, W, and the bits of the float32 scale (in (0, 16]).
 * roi_pool_forward: out [R,C,P,P] in the maps' type = roi_align of box r on the map of its level and image, float32 arithmetic:
 *   start = lo * scale - .5, roi = (hi * scale - .5) - start, bin = roi / P, grid = sampling_ratio or ceil(bin) when it is 0, a sample at
 *   start + p * bin + (i + .5) * bin / grid, 0 outside [-1, size], clamped to [0, size - 1], bilinear taps, the mean over grid_h * grid_w.
 *   Evaluated separably, sum_y Ay[ph,y] * (sum_x Ax[pw,x] * F[c,y,x]) / count with Ay, Ax the summed tap weights (csrc/roi_pool.hip).
 *   A refused box, a level outside [0, n_levels) and roi <= 0 on an axis give a zero row.  One launch for all levels and images.
 * roi_pool_backward: the pointers in levels are the GRADIENT maps, written whole (zeros included, no memset needed) with
 *   grad[n,c,y,x] = the sum over the boxes r of image n and that level, in index order, ph outer and pw inner, of
 *   ((Ay[ph,y] * Ax[pw,x]) / count_r) * grad_out[r,c,ph,pw]; a NULL pointer skips the level.  first: as above or NULL (then
 *   every workgroup looks at all R rows).  No float atomics: the same input gives the same bytes on every run.
 * 1 <= P <= 64; 0 <= sampling_ratio <= 1024; the two axis tables take 4 * (H + W) + 64 * P + 1112 bytes of LDS for the largest H and W, at
 * most 64 KiB (else UMR_ERR_INVALID); the backward stages a box's output gradients there too, 128 * P * P bytes, when P <= 16 and they
 * fit.  No synchronisation, nothing allocated. */
int umr_roi_pool_prepare(const float* boxes, int box_stride, int64_t R, const int32_t* first, int64_t N, int n_levels, int min_level,
                         int max_level, float canonical_box_size, int canonical_level, int32_t* info, umr_stream_t stream);
int umr_roi_pool_forward(const int64_t* levels, int n_levels, int64_t N, int C, int dtype, const float* boxes, int box_stride,
                         const int32_t* info, int64_t R, int P, int sampling_ratio, void* out, umr_stream_t stream);
int umr_roi_pool_backward(const int64_t* levels, int n_levels, int64_t N, int C, int dtype, const float* boxes, int box_stride,
                          const int32_t* info, const int32_t* first, int64_t R, int P, int sampling_ratio, const void* grad_out,
                          umr_stream_t stream);

/* ---- the RPN's proposal step (cad/modeling/meta_arch/rcnn.py:165, 213, 333 -> Detectron2's RPN.predict_proposals: _decode_proposals +
 * find_top_rpn_proposals; csrc/rpn.hip) -------------------------------------------------------------------------------------------------
 * levels: a HOST array of 5 int64 per level, at most 8 levels, copied into the kernels' arguments by value: the pointers of the level's
 *   objectness logits [N,A,H,W] and anchor deltas [N,4A,H,W] (channel a * 4 + c; both UMR_F32 or both UMR_BF16, contiguous, read in
 *   place), H, W and the stride (H * W * A < 2^31; H * stride, W * stride <= 2^24).  A <= 16.  cells: float32 [n_levels,16,4] on the device,
 *   the cell anchors of level l in rows [0, A); image_sizes: float32 [N,2] = (h, w) on the device.
 * Per (image, level): the K = min(H * W * A, pre_nms_topk) (<= 4096) largest logits over f = (y * W + x) * A + a in torch.topk's order
 *   (NaN above +inf, -0.0 == +0.0), equal values in ascending f; anchor (x * stride + offset * stride, y * stride + offset * stride, ...) +
 *   cell (offset * stride must be a float32 value); Box2BoxTransform.apply_deltas with weights (wx, wy, ww, wh); a candidate with a
 *   non-finite coordinate or logit is dropped (flag 1); clip to (h, w); dropped unless x2 - x1 > min_box_size and y2 - y1 > min_box_size (flag 2); greedy NMS within the level in
 *   that order (iou > nms_thresh, det_select's formula); the survivors of an image by descending logit, then level, then rank, the
 *   first cap = min(post_nms_topk, sum of K) to out_boxes [N,cap,4] / out_logits [N,cap] (rows past counts[n] are NOT written).  The
 *   float32 operation order is written out in csrc/rpn.hip.
 * cand_* [N, sum of K] (boxes and raw x 4; raw may be NULL): every level's candidates in rank order, level after level: the clipped box,
 *   the logit, f, the flag, and the box before the clip.  stats int32 [N,n_levels,5]: candidates, non-finite, empty, suppressed, kept by
 *   the NMS.  phases: 1 = the partial selects of levels above 16384 scores, 2 = select + rank + decode, 4 = the suppression matrices,
 *   8 = the scans, 16 = the merge; 31 = all (five launches).  workspace >= rpn_workspace(...) bytes, 16-byte aligned.  Nothing is read
 *   back; no float atomics. */
int64_t umr_rpn_workspace(const int64_t* levels, int n_levels, int64_t N, int A, int pre_nms_topk);
int umr_rpn_proposals(const int64_t* levels, int n_levels, int64_t N, int A, int dtype, const float* cells, const float* image_sizes,
                      int pre_nms_topk, int post_nms_topk, float nms_thresh, float min_box_size, float wx, float wy, float ww, float wh,
                      double offset, int phases, float* cand_boxes, float* cand_scores, int32_t* cand_idx, uint8_t* cand_flags,
                      float* cand_raw, float* out_boxes, float* out_logits, int32_t* counts, int32_t* stats, void* workspace,
                      int64_t workspace_bytes, umr_stream_t stream);

/* ---- the RPN's training half (cad/modeling/meta_arch/rcnn.py:165, 333 -> Detectron2's RPN.label_and_sample_anchors and RPN.losses;
 * csrc/rpn_loss.hip) -----------------------------------------------------------------------------------------------------------------------
 * Anchors as above, never as a tensor: anchor r of an image = level after level, inside a level f = (y * W + x) * A + a; R per image
 *   (R < 2^31 - 1).  cells: float32 [n_levels,16,4], image_sizes: float32 [N,2] = (h, w), gt_boxes: float32 [n_gt,4] = the images' ground
 *   truths one after the other, gt_first: int32 [N+1] their prefix table; all on the device.
 * rpn_label_sample, levels: a HOST array of 3 int64 per level (H, W, stride), by value into the kernels' arguments.
 *   match   matched_vals / matched_idxs [N,R]: the maximum IoU (box_loss's formula: 0 unless inter > 0, correctly rounded division, bit
 *           for bit a float32 NumPy value) over the image's ground truths and the FIRST index reaching it; row_max float32 [n_gt]: each
 *           ground truth's maximum over the anchors (0 when it overlaps none).  A ground truth with a non-finite coordinate takes no part
 *           and is counted (a departure from Detectron2, which would hand the NaN on).
 *   label   labels int8 [N,R] BEFORE sampling: v < iou_lo: 0, v < iou_hi: -1, else 1; all 0 for an image without usable ground truths;
 *           allow_low_quality: 1 as well where the anchor's IoU with some ground truth equals that row's maximum, exactly (the matched
 *           index is not changed; a row maximum of 0 marks every anchor of IoU 0 with that ground truth: Detectron2's quirk);
 *           boundary_thresh t >= 0: -1 unless x1 >= -t, y1 >= -t, x2 < w + t, y2 < h + t.
 *   select  P, Q = the numbers of labels 1 and 0; num_pos = min(P, pos_cap), num_neg = min(Q, batch_size - num_pos); the num_pos (num_neg)
 *           anchors of label 1 (0) with the largest key, equal keys to the lower r.  key = keys[n,r] & 0x7fffffff (keys int32 [N,R]) or,
 *           keys == NULL, fmix(fmix(r ^ seed_lo) ^ (n * 0x9e3779b9 + seed_hi)) >> 1 with murmur3's 32-bit finaliser fmix and the halves
 *           of seed.  sample_index int32 [N,batch_size]: r of the positives ascending, then of the negatives ascending; sample_gt: their
 *           matched_idxs; counts int32 [N,2] = (num_pos, num_neg); entries past the counts are not written.  dense_labels int8 [N,R] or
 *           NULL: the labels AFTER sampling (-1 for every anchor not sampled).
 *   counters int32 [N,5]: P, Q, num_pos, num_neg, bad ground truths.  phases: 1 = match (zeroes counters and row_max first), 2 = label,
 *   4 = the partial selects when R > 16384 (one workgroup per 16384 anchors, class and image), 8 = select; 15 = all (three or four
 *   launches).  batch_size <= 1024.  workspace >= rpn_label_workspace(...) bytes (0 when R <= 16384), never NULL, 4-byte aligned.
 * rpn_loss, levels: 7 int64 per level (H, W, stride, logits [N,A,H,W], deltas [N,4A,H,W], and the two gradient maps of the same shapes
 *   and type, which the CALLER ZEROED: the launch stores only at the samples).  float64 arithmetic on the float32 anchors and widened
 *   predictions: losses[0] = scale_cls * sum over the samples of binary_cross_entropy_with_logits(x, label), losses[1] = scale_loc * sum
 *   over the sampled positives of smooth_l1(deltas - get_deltas(anchor, matched ground truth), beta) (beta < 1e-5: L1, gradient 0 at 0);
 *   the gradient maps receive d losses[0] / d logits and d losses[1] / d deltas.  phases: 1 = terms, gradients and per-image partial
 *   sums, 2 = the sum over the images in index order; 3 = all.  workspace >= rpn_loss_workspace(N) bytes, 8-byte aligned.
 * No synchronisation, nothing read back, nothing allocated, no float atomics. */
int64_t umr_rpn_label_workspace(const int64_t* levels, int n_levels, int64_t N, int A, int batch_size);
int umr_rpn_label_sample(const int64_t* levels, int n_levels, int64_t N, int A, const float* cells, const float* image_sizes,
                         const float* gt_boxes, const int32_t* gt_first, int64_t n_gt, float iou_lo, float iou_hi, int allow_low_quality,
                         int batch_size, int pos_cap, float boundary_thresh, double offset, int64_t seed, const int32_t* keys, int phases,
                         float* matched_vals, int32_t* matched_idxs, float* row_max, int8_t* labels, int32_t* sample_index,
                         int32_t* sample_gt, int32_t* counts, int8_t* dense_labels, int32_t* counters, void* workspace,
                         int64_t workspace_bytes, umr_stream_t stream);
int64_t umr_rpn_loss_workspace(int64_t N);
int umr_rpn_loss(const int64_t* levels, int n_levels, int64_t N, int A, int dtype, const float* cells, const float* gt_boxes,
                 const int32_t* gt_first, int64_t n_gt, const int32_t* sample_index, const int32_t* sample_gt, const int32_t* counts,
                 int batch_size, float wx, float wy, float ww, float wh, float smooth_l1_beta, double scale_cls, double scale_loc,
                 double offset, int phases, float* losses, void* workspace, int64_t workspace_bytes, umr_stream_t stream);

/* ---- the ROI heads' proposal sampling (cad/modeling/roi_heads/roi_heads.py:207-328 -> Detectron2's ROIHeads.label_and_sample_proposals
 * with add_ground_truth_to_proposals, Matcher([t], [0, 1]) and subsample_labels; csrc/roi_sample.hip) -----------------------------------
 * table: int64 [n_images,11] ON THE DEVICE, per image: the addresses of proposal_boxes float32 [R,4], objectness_logits float32 [R],
 *   gt_boxes float32 [G,4], gt_classes int64 [G], gt_scores float32 [G] or 0, keys int32 [R+A] or 0; then R, G, A (G when the ground
 *   truths are appended, else 0), chunk_first and cand_first.  Candidate r of an image: proposal r for r < R, ground truth r - R for
 *   R <= r < R + A, read in place; R + A <= 16384.  The candidates of all images one after the other: n_cand in all, image n's at
 *   cand_first, cut into chunks of 256 per image (chunk_first, n_chunks in all; an image without candidates shares its chunk_first with
 *   the next one).
 *   match   per candidate the maximum IoU (box_loss's formula, bit for bit a float32 NumPy value) over the image's ground truths and the
 *           LOWEST index attaining it; a NaN never wins; foreground iff the maximum >= iou_threshold; class = gt_classes[matched] or
 *           num_classes; an image without ground truths: all background, index 0.  A candidate with a non-finite coordinate is counted
 *           (`bad`) and never sampled (a departure from Detectron2, whose Matcher would label the NaN row foreground).
 *   select  subsample_labels: positive iff class != -1 and != num_classes, negative iff class == num_classes, P and Q of them; num_pos =
 *           min(P, pos_cap), num_neg = min(Q, batch_size - num_pos); the num_pos (num_neg) candidates with the largest key, equal keys to
 *           the lower r.  key = keys[r] & 0x7fffffff or, without keys, rpn_label_sample's hash of (seed, image, r); the caller salts the
 *           seed.  Row order: the positives, then the negatives; inside each by_key ? (key descending, r ascending) : r ascending.
 *   out_* [n_images,batch_size,...]: proposal boxes and logits (gt_logit for an appended ground truth), classes int64, the matched
 *           ground truth's box and score (zero in an image without ground truths; out_gt_scores may be NULL) on EVERY row, the matched
 *           index int64, the sampled r int32; rows past num_pos + num_neg are zero with class -1.  counts int32 [n_images,2] = (num_pos,
 *           num_neg); counters int32 [n_images,5] = P, Q, num_pos, num_neg, bad.
 *   phases: 1 = match, 2 = select + order + gather; 3 = all (two launches).  batch_size <= 1024.  workspace >= roi_sample_workspace(n_cand)
 *   bytes, 4-byte aligned.  No synchronisation, nothing read back, nothing allocated, no atomics on memory: the same input, the same bytes. */
int64_t umr_roi_sample_workspace(int64_t n_cand);
int umr_roi_sample(const int64_t* table, int n_images, int64_t n_cand, int64_t n_chunks, float iou_threshold, int64_t num_classes,
                   int batch_size, int pos_cap, int by_key, float gt_logit, int64_t seed, int phases, float* out_boxes, float* out_logits,
                   int64_t* out_classes, float* out_gt_boxes, float* out_gt_scores, int64_t* out_matched_idxs, int32_t* out_sampled_idxs,
                   int32_t* counts, int32_t* counters, void* workspace, int64_t workspace_bytes, umr_stream_t stream);

/* ---- the detector's input path (cad/data/dataset_mapper.py:152-213 with ResizeShortestEdge + RandomFlip, cad/data/transforms/
 * transform.py:94-163, GeneralizedRCNN.preprocess_image, cad/modeling/meta_arch/rcnn.py:229-240; csrc/det_input.hip) ----------------------
 * Three entries, each ONE launch for a whole ragged batch of B images.  desc: int64 [B][fields] ON THE DEVICE (addresses as integers);
 * tab: int32 [tab_len] on the device, the tables the descriptors point into by element offset.  The host builds the tables in float64
 * (unmore_amd/detector_input.py); the device side is integer only, so the bytes are PIL's.
 * det_resize_bilinear  PIL Image.resize(BILINEAR) on 8-bit RGB, HWC in, planar CHW out, flip at the store.  desc [B][16]: src u8 [H,W,3],
 *   dst u8 [3,nh,nw], H, W, nh, nw, flip (1 horizontal, 2 vertical), then per axis (horizontal: 7-9, vertical: 10-12) the offset of
 *   its (lo, n) pairs [out][2], of its weights [out][ksize] (22 fractional bits) and ksize; TH, TW (output tile, TW <= 64, the input rows
 *   a tile reads times TW <= 10880) and the image's first tile; total_tiles = the grid.  byte = clip((2^21 + sum_j in[lo + j] * k_j) >>
 *   22), horizontal pass first, its bytes staged in LDS.  An axis that keeps its size: lo = i, n = 1, k = 2^22.
 * det_resize_nearest   PIL Image.resize(NEAREST) of N masks per image, any non-zero input byte = set, 0 / 1 bytes out.  desc [B][13]:
 *   src (mask n at src + n * stride), dst u8 [N,nh,nw], N, H, W, nh, nw, flip, the offsets of the column table [nw] and the row table
 *   [nh] (source indices), the image's first flag, its first workgroup (a workgroup owns ceil(4096 / nw) rows, rounded up to a
 *   multiple of 4, of one mask;
 *   total_blocks = the grid), stride.  flags int32 [n_flags], ZEROED by the caller: flag |= 1 iff the resized mask has a set pixel (one
 *   integer atomic OR per workgroup).
 * det_normalize_pad    out float32 [B,3,Hp,Wp], 16-byte aligned: (float32(u8) - mean[c]) / std[c] (IEEE divide) at the top left, pad_value
 *   elsewhere; every element is written.  desc [B][4]: src u8 [3,h,w], h, w, 0.
 * A descriptor that breaks its own bounds (sizes, table slices past tab_len, flags past n_flags, a tile that does not fit) is skipped;
 * an index read from a table is checked before it is used.  No synchronisation, nothing allocated; the same input, the same bytes. */
int umr_det_resize_bilinear(const int64_t* desc, int B, const int32_t* tab, int64_t tab_len, int64_t total_tiles, umr_stream_t stream);
int umr_det_resize_nearest(const int64_t* desc, int B, const int32_t* tab, int64_t tab_len, int64_t total_blocks, int32_t* flags,
                           int64_t n_flags, umr_stream_t stream);
int umr_det_normalize_pad(const int64_t* desc, int B, int Hp, int Wp, float mean0, float mean1, float mean2, float std0, float std1,
                          float std2, float pad_value, float* out, umr_stream_t stream);

/* ---- the tail of the detector's mask head (cad/modeling/roi_heads/roi_heads.py:1098-1201, CustomMaskRCNNConvUpsampleHead: the 1x1
 * predictor on the ReLU'd 2x2 stride-2 deconvolution; csrc/mask_head.hip) ------------------------------------------------------------------
 * D [M, 4C] (UMR_F32 / UMR_BF16, contiguous, 16-byte aligned) is the deconvolution GEMM's output after bias and ReLU, as umr_gemm_nt
 *   stores it: M = R * S * S, row m = (r * S + y) * S + x, column n = (2 * ky + kx) * C + co.  The [R,2S,2S,C] map is never laid out.
 *   wp: float32 [C], bp: float32 [1], both on the device.
 * mask_head_logits: logits [R,1,2S,2S] (the type of D, or float32 with out_f32) = bp + sum_co D[m,(ky,kx,co)] * wp[co] at (r, 2y + ky,
 *   2x + kx), summed in float32 in an order that depends on C and the type alone; sigmoid != 0 stores 1 / (1 + exp(-logit)) instead
 *   (mask_rcnn_inference).
 * mask_head_tail_bwd: dlogits [R,1,2S,2S] (the type of D, or float32 with dlogits_f32).  D is OVERWRITTEN with
 *   G[m,(ky,kx,co)] = D > 0 ? dlogit * wp[co] : 0, the float32 product rounded once to the type of D; dwp float32 [C] = sum over m and
 *   the taps of dlogit * D[m,(tap,co)], dbp float32 [1] = sum of dlogits.  phases: 1 = G and one float32 partial sum per channel and
 *   workgroup of 256 rows, 2 = the partials added in a fixed order; 3 = both.  workspace >= mask_head_workspace(M, C) bytes (-1 for
 *   arguments the launch would refuse), 4-byte aligned.
 * C a multiple of 64, at most 1024, and 1 <= S <= 64 (else UMR_ERR_UNSUPPORTED); R * S * S < 2^31.  R == 0 is a no-op (tail_bwd with
 *   phase 2 then stores zeros).  No float atomics, no synchronisation, nothing allocated; the same input gives the same bytes on every run. */
int64_t umr_mask_head_workspace(int64_t M, int C);
int umr_mask_head_logits(const void* D, const float* wp, const float* bp, void* logits, int64_t R, int S, int C, int dtype,
                         int out_f32, int sigmoid, umr_stream_t stream);
int umr_mask_head_tail_bwd(void* D, const void* dlogits, int dlogits_f32, const float* wp, float* dwp, float* dbp, void* workspace,
                           int64_t workspace_bytes, int64_t R, int S, int C, int dtype, int phases, umr_stream_t stream);

/* ---- the predictors of the RPN head (Detectron2's StandardRPNHead: the 1x1 objectness_logits and anchor_deltas convolutions on the
 * ReLU'd 3x3 convolution, the same weights on every level; csrc/rpn_head.hip) ------------------------------------------------------------
 * T [M, C] (UMR_F32 / UMR_BF16, contiguous, 16-byte aligned) is the hidden map of ALL levels stacked, NHWC: level l starts at row
 *   first_l = sum over the earlier levels of N * H * W, its row (n * H_l + y) * W_l + x.  levels: 4 int64 per level ON THE HOST:
 *   H, W, and the device pointers of the level's two contiguous NCHW maps [N, A, H, W] and [N, 4A, H, W].  wo float32 [A, C],
 *   bo float32 [A], wd float32 [4A, C], bd float32 [4A], on the device; the products read them rounded to the compute type.
 * rpn_head_predict: logits[l][n, a, y, x] = bo[a] + sum_c T[m, c] wo[a, c], deltas[l][n, j, y, x] = bd[j] + sum_c T[m, c] wd[j, c],
 *   float32 sums on the matrix cores, stored in the type of T or as float32 (out_f32).  T is only read.  One launch for all levels.
 * rpn_head_predict_bwd: the maps are the incoming gradients dlogits / ddeltas, in the type of T or float32 (grads_f32).  T is
 *   OVERWRITTEN with G[m, c] = T[m, c] > 0 ? sum_{j < 5A} g[m, j] w[j, c] : 0 rounded once to the type of T; dwo / dbo / dwd / dbd
 *   float32 in the shapes of wo / bo / wd / bd: sum_m g[m, j] T[m, c] and sum_m g[m, j].  With UMR_BF16 the gradients are rounded to
 *   bfloat16 before the products (also float32 ones); the bias sums take them as they are.  phases: 1 = G and one float32 partial
 *   [16][C + 1] per workgroup, 2 = the partials added in a fixed order; 3 = both.  The grid is min(ceil(M / 128), 512) workgroups, a
 *   function of M alone.  workspace >= rpn_head_workspace(M, C, A) bytes (-1 for shapes the launch would refuse), 4-byte aligned.
 * 1 <= A <= 3 (5A <= 16), C a multiple of 64 up to 1024, 1 <= n_levels <= 8 (else UMR_ERR_UNSUPPORTED); M < 2^31.  M == 0 is a no-op
 *   (predict_bwd with phase 2 then stores zeros).  No float atomics, no synchronisation, nothing allocated: the same input gives the
 *   same bytes on every run and every device. */
int64_t umr_rpn_head_workspace(int64_t M, int C, int A);
int umr_rpn_head_predict(const void* T, const int64_t* levels, int n_levels, int64_t N, int C, int A, const float* wo, const float* bo,
                         const float* wd, const float* bd, int dtype, int out_f32, umr_stream_t stream);
int umr_rpn_head_predict_bwd(void* T, const int64_t* levels, int n_levels, int64_t N, int C, int A, int grads_f32, const float* wo,
                             const float* wd, float* dwo, float* dbo, float* dwd, float* dbd, void* workspace, int64_t workspace_bytes,
                             int dtype, int phases, umr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
