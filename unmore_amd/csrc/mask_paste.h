// The paste arithmetic of object scoring, shared by reasoning.hip (umr_mask_paste_stats, umr_mask_paste) and rle.hip
// (umr_mask_paste_rle): one definition, so that every kernel decides a pasted pixel with the same instructions.
#pragma once
#include "umr_common.h"

// ---- object scoring (object_scoring.py:172-272): the two binary masks of a proposal (||center|| > 0.5, sigmoid(sdf) > 0.5, on its
// S x S crop) are resized to the proposal's box with torchvision's tensor Resize -- for an integer tensor: bilinear in f32
// (align_corners=False), then torch.round (half to even: 1 iff the value exceeds 0.5) -- pasted into an image-sized canvas and OR-ed
// (:196-228).  Both masks live in LDS as bytes; the bilinear arithmetic is PyTorch's, unfused: h0 * (w0 * p00 + w1 * p01) + h1 * (...).
struct PasteAxis { int i0, i1; float l0, l1; };
__device__ __forceinline__ PasteAxis paste_axis(int o, int out_size, int S) {
    const float scale = (float)S / (float)out_size;
    const float src = fmaxf(__fsub_rn(__fmul_rn(scale, (float)o + 0.5f), 0.5f), 0.f);
    int i0 = (int)floorf(src);
    if (i0 > S - 1) i0 = S - 1;
    const float l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
    return PasteAxis{i0, i0 < S - 1 ? i0 + 1 : i0, __fsub_rn(1.f, l1), l1};
}
__device__ __forceinline__ bool paste_bit(const unsigned char* m, int S, const PasteAxis& ay, const PasteAxis& ax) {
    const float p00 = (float)m[ay.i0 * S + ax.i0], p01 = (float)m[ay.i0 * S + ax.i1];
    const float p10 = (float)m[ay.i1 * S + ax.i0], p11 = (float)m[ay.i1 * S + ax.i1];
    const float top = __fadd_rn(__fmul_rn(ax.l0, p00), __fmul_rn(ax.l1, p01));
    const float bot = __fadd_rn(__fmul_rn(ax.l0, p10), __fmul_rn(ax.l1, p11));
    return __fadd_rn(__fmul_rn(ay.l0, top), __fmul_rn(ay.l1, bot)) > 0.5f;
}
// fills the two LDS mask planes of proposal b; returns (this thread's) partial maxima of ||center|| and sdf
__device__ __forceinline__ void paste_masks_to_lds(const float* __restrict__ sdf, const float* __restrict__ center, int b, int S, unsigned char* mc,
                                                   unsigned char* mb, float& max_norm, float& max_sdf) {
    const int SS = S * S;
    const float* s = sdf + (int64_t)b * SS;
    const float* c0 = center + (int64_t)b * 2 * SS;
    const float* c1 = c0 + SS;
    for (int i = threadIdx.x; i < SS; i += blockDim.x) {
        const float sv = s[i];
        const float sg = 1.0f / (1.0f + expf(-sv));
        const float nr = sqrtf(c0[i] * c0[i] + c1[i] * c1[i]);
        mc[i] = nr > 0.5f ? 1 : 0;
        mb[i] = sg > 0.5f ? 1 : 0;
        max_norm = fmaxf(max_norm, nr);
        max_sdf = fmaxf(max_sdf, sv);
    }
}
