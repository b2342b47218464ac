// The box geometry, the grid anchors and the sampling hash that the detector's kernels share (box_loss.hip, rpn.hip,
// rpn_loss.hip, roi_sample.hip, det_post.hip, nms.hip).  These functions carry the bit-exactness contract with Detectron2 and torchvision: which
// IoU form hands a NaN on, the correctly rounded divisions, the float32 value of log(1000 / 16), the hash that draws the
// samples.  Each is written once, here.
//
// Include this header only after `#pragma clang fp contract(off)`, which every file that uses it has as its first line: all arithmetic
// below is float32 with every operation rounded on its own, and a single fused multiply-add (in a * b + c the product would no longer
// be rounded) changes the bits that the tests compare against NumPy restatements of the references.
#pragma once
#include "umr_common.h"
#include <float.h>

constexpr int GRID_MAX_A = 16;                        // cell anchors per level in the uploaded `cells` table [L, GRID_MAX_A, 4]
constexpr float BOX_SCALE_CLAMP = (float)4.135166556742356;   // log(1000 / 16) rounded to float32, as torch.clamp rounds the scalar

__device__ __forceinline__ bool box_finite(float v) { return fabsf(v) <= FLT_MAX; }      // false for NaN and +-inf

__device__ __forceinline__ float box_clip(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }   // a NaN stays a NaN

__device__ __forceinline__ float box_area(float x1, float y1, float x2, float y2) { return (x2 - x1) * (y2 - y1); }

// ---------------------------------------------------------------------------------------------------------------- the two IoU forms
// They differ on purpose, in what a NaN coordinate and an empty union do, because the two references differ.
//
// The matcher's form (Detectron2's pairwise_iou, which the Matcher of the RPN and of the ROI heads reads):
//   iou(a, b) = inter > 0 ? inter / ((area_a + area_b) - inter) : 0,  inter = max(min(a.x2, b.x2) - max(a.x1, b.x1), 0) * (same in y);
// the division is correctly rounded, so the value equals a float32 NumPy restatement bit for bit.
__device__ __forceinline__ float box_iou_match(float ax1, float ay1, float ax2, float ay2, float a_area, float bx1, float by1, float bx2,
                                               float by2, float b_area) {
    // torch.min / torch.max hand a NaN on (fminf / fmaxf would drop it): a NaN coordinate ends as inter > 0 == false, an IoU of 0
    const float x_hi = (ax2 != ax2 || ax2 < bx2) ? ax2 : bx2, x_lo = (ax1 != ax1 || ax1 > bx1) ? ax1 : bx1;
    const float y_hi = (ay2 != ay2 || ay2 < by2) ? ay2 : by2, y_lo = (ay1 != ay1 || ay1 > by1) ? ay1 : by1;
    float w = x_hi - x_lo, h = y_hi - y_lo;
    w = w > 0.f ? w : 0.f;
    h = h > 0.f ? h : 0.f;
    const float inter = w * h;
    return inter > 0.f ? __fdiv_rn(inter, (a_area + b_area) - inter) : 0.f;
}

// The suppression's form (torchvision's nms kernel; called from nms_bitmask.h alone, which every NMS here runs on): std::max / std::min
// written as fmaxf / fminf,
//   w = max(0, min(a.x2, b.x2) - max(a.x1, b.x1)), h likewise, inter = w * h, iou = inter / ((area_a + area_b) - inter),
// correctly rounded and with no test of inter: two empty boxes give 0 / 0 = NaN, and `iou > nms_thresh` is then false (not suppressed).
__device__ __forceinline__ float box_iou_nms(const f32x4 a, float a_area, const f32x4 b) {
    const float xx1 = fmaxf(a[0], b[0]), yy1 = fmaxf(a[1], b[1]), xx2 = fminf(a[2], b[2]), yy2 = fminf(a[3], b[3]);
    const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
    const float inter = w * h;
    const float b_area = box_area(b[0], b[1], b[2], b[3]);
    return __fdiv_rn(inter, (a_area + b_area) - inter);
}

// ---------------------------------------------------------------------------------------------------------------- Box2BoxTransform
// w: the transform's weights (wx, wy, ww, wh).
// apply_deltas: w = x2 - x1; cx = x1 + .5 w; dx = dx / wx; dw = min(dw / ww, log(1000 / 16)); pcx = dx * w + cx; pw = expf(dw) * w;
// x1' = pcx - .5 pw; x2' = pcx + .5 pw
__device__ __forceinline__ void box_apply_deltas(const float d[4], const float b[4], const float w[4], float out[4]) {
    const float bw = b[2] - b[0], bh = b[3] - b[1];
    const float cx = b[0] + .5f * bw, cy = b[1] + .5f * bh;
    const float dx = __fdiv_rn(d[0], w[0]), dy = __fdiv_rn(d[1], w[1]);
    float dw = __fdiv_rn(d[2], w[2]), dh = __fdiv_rn(d[3], w[3]);
    dw = dw > BOX_SCALE_CLAMP ? BOX_SCALE_CLAMP : dw;                     // a NaN stays a NaN, as torch.clamp leaves it
    dh = dh > BOX_SCALE_CLAMP ? BOX_SCALE_CLAMP : dh;
    const float pcx = dx * bw + cx, pcy = dy * bh + cy;
    const float pw = expf(dw) * bw, ph = expf(dh) * bh;
    out[0] = pcx - .5f * pw;
    out[1] = pcy - .5f * ph;
    out[2] = pcx + .5f * pw;
    out[3] = pcy + .5f * ph;
}

// get_deltas: dx = wx * (tcx - scx) / sw; dw = ww * logf(tw / sw).
// false: an extent that Detectron2 would assert on (source) or take the logarithm of (target) is not positive, or something is not finite
__device__ __forceinline__ bool box_get_deltas(const float s[4], const float t[4], const float w[4], float out[4]) {
    const float sw = s[2] - s[0], sh = s[3] - s[1];
    const float scx = s[0] + .5f * sw, scy = s[1] + .5f * sh;
    const float tw = t[2] - t[0], th = t[3] - t[1];
    const float tcx = t[0] + .5f * tw, tcy = t[1] + .5f * th;
    out[0] = __fdiv_rn(w[0] * (tcx - scx), sw);
    out[1] = __fdiv_rn(w[1] * (tcy - scy), sh);
    out[2] = w[2] * logf(__fdiv_rn(tw, sw));
    out[3] = w[3] * logf(__fdiv_rn(th, sh));
    return sw > 0.f && sh > 0.f && tw > 0.f && th > 0.f && box_finite(out[0]) && box_finite(out[1]) && box_finite(out[2]) &&
           box_finite(out[3]);
}

// ---------------------------------------------------------------------------------------------------------------- grid anchors
// Detectron2's DefaultAnchorGenerator: the anchor at position (x, y) of a level for the cell anchor `cell` (four floats of the level's
// row of the `cells` table, cells + (level * GRID_MAX_A + a) * 4); off = offset * stride, exact.
//   sx = float(x * stride) + off, sy = float(y * stride) + off;  (sx + c0, sy + c1, sx + c2, sy + c3)
__device__ __forceinline__ void grid_anchor(const float* __restrict__ cell, int x, int y, int stride, float off, float b[4]) {
    const float sx = (float)(x * stride) + off, sy = (float)(y * stride) + off;
    b[0] = sx + cell[0]; b[1] = sy + cell[1]; b[2] = sx + cell[2]; b[3] = sy + cell[3];
}

// ---------------------------------------------------------------------------------------------------------------- the sampling hash
// murmur3's 32-bit finaliser, mod 2^32
__device__ __forceinline__ unsigned hash_fmix(unsigned h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// The 31-bit key that draws entry r of image `image`, s_lo / s_hi the low / high 32 bits of the seed:
//   key = fmix(fmix(r ^ s_lo) ^ (image * 0x9e3779b9 + s_hi)) >> 1
__device__ __forceinline__ unsigned sample_key(unsigned r, unsigned image, unsigned s_lo, unsigned s_hi) {
    return hash_fmix(hash_fmix(r ^ s_lo) ^ (image * 0x9e3779b9u + s_hi)) >> 1;
}
// The same key for a caller that formed its image's part of it once: mix = sample_mix(image, s_hi) (image 0 leaves mix as it is).
__device__ __forceinline__ unsigned sample_mix(unsigned image, unsigned s_hi) { return image * 0x9e3779b9u + s_hi; }
__device__ __forceinline__ unsigned sample_key_mixed(unsigned r, unsigned s_lo, unsigned mix) { return sample_key(r, 0u, s_lo, mix); }
