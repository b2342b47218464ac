// Greedy non-maximum suppression as a bit matrix, for the three callers that follow torchvision.ops.nms: the proposals of a pyramid
// level (rpn.hip), the detections of an image (det_post.hip, with classes) and the boxes of object discovery and scoring (nms.hip).
//
// The specification, stated once.  The candidates stand in rank order: descending score, the caller's order among equal scores.
// Rank i suppresses rank j iff j > i, the caller's predicate holds (always, or "same class") and box_iou_nms(i, j) > thresh --
// strict, in float32, with every operation rounded on its own (det_box.h); two empty boxes give 0 / 0 = NaN, which does not
// suppress.  Walking the ranks in order, a rank that is valid and not yet suppressed is kept and suppresses; nothing else does.
//
// Two steps.  The mask: one wave per 64 x 64 tile of the upper triangle; nms_tile_word gives a row's word of a tile, bit jj =
// "rank i suppresses rank j0 + jj".  Only the words on and right of a row's diagonal word are ever written or read.  The scan: one
// wave walks the ranks 64 at a time, nms_greedy_scan.
//
// Include only after `#pragma clang fp contract(off)` and after det_box.h.
#pragma once
#include "det_box.h"

// lane `src` (wave-uniform) of a 64-bit value, through the scalar unit: no LDS round trip on the scan's serial chain
__device__ __forceinline__ unsigned long long nms_lane_value(unsigned long long v, int src) {
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, src), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

struct NmsAlways {
    __device__ __forceinline__ bool operator()(int) const { return true; }
};

// word of row box `a` (rank i) against the nj staged column boxes of ranks j0 ...; pred(jj): may column jj be suppressed by this row
template <typename Pred>
__device__ __forceinline__ unsigned long long nms_tile_word(const f32x4 a, int i, const f32x4* tile, int j0, int nj, float thresh, Pred pred) {
    const float a_area = box_area(a[0], a[1], a[2], a[3]);
    unsigned long long bits = 0ull;
    for (int jj = 0; jj < nj; ++jj) {
        const f32x4 b = tile[jj];
        const float iou = box_iou_nms(a, a_area, b);
        if (j0 + jj > i && iou > thresh && pred(jj)) bits |= 1ull << jj;    // pred last: before the IoU, "always" compiles to a branch per column
    }
    return bits;
}

// the all-ones valid set of n ranks: word `word` of it
__device__ __forceinline__ unsigned long long nms_all_valid(int word, int n) {
    const int left = n - word * 64;
    return left >= 64 ? ~0ull : (left > 0 ? (1ull << left) - 1ull : 0ull);
}

// The walk, by one wave of 64 lanes, wave-uniform throughout.  WPL words of the removed set per lane: lane l holds the words
// l + 64 q, so n <= 4096 WPL.  Row r of the matrix starts at mat + r * pitch; its words [r / 64, words) were written.  valid[q]: the
// lane's words of the ranks that may be kept at all, zero from rank n on.  The first min(kept, limit) kept ranks go to kept_rank
// (LDS, room for n) in ascending order and their number is returned: stopping after `limit` kept ranks gives exactly the first
// `limit` entries of the full list, so the walk leaves at the first block boundary with kept >= limit and the count is clamped.
//
// Inside a block of 64 ranks the walk runs on the diagonal tile held in registers (a rank that is valid and not removed is kept and
// removes its row's bits); then the kept rows are ORed into the words after the block with their loads in flight together.
template <int WPL>
__device__ __forceinline__ int nms_greedy_scan(const unsigned long long* __restrict__ mat, int pitch, int words, int n,
                                               const unsigned long long (&valid)[WPL], int limit, int* kept_rank) {
    const int lane = threadIdx.x;
    unsigned long long rem[WPL];                                    // words lane + 64 q of the removed set
#pragma unroll
    for (int q = 0; q < WPL; ++q) rem[q] = 0ull;
    int kept = 0;
    for (int w = 0; w < words && kept < limit; ++w) {               // 64 ranks at a time
        unsigned long long cur = 0ull;
#pragma unroll
        for (int q = 0; q < WPL; ++q)
            if (WPL == 1 || (w >> 6) == q) cur = nms_lane_value(valid[q], w & 63) & ~nms_lane_value(rem[q], w & 63);
        if (!cur) continue;
        // the diagonal tile in registers: lane b holds word w of row 64 w + b, the ranks of this block that rank 64 w + b removes
        const int ib = w * 64 + lane;
        const unsigned long long diag = ib < n ? mat[(long long)ib * pitch + w] : 0ull;
        unsigned long long keep = 0ull;
        while (cur) {                                               // the greedy walk inside the block: no memory on the chain
            const int b = __ffsll((long long)cur) - 1;
            keep |= 1ull << b;
            cur &= ~(nms_lane_value(diag, b) | (1ull << b));        // a row holds only bits above its own rank
        }
        if ((keep >> lane) & 1ull) kept_rank[kept + __popcll(keep & ((1ull << lane) - 1ull))] = ib;
        kept += __popcll(keep);
#pragma unroll
        for (int q = 0; q < WPL; ++q) {
            const int col = lane + 64 * q;
            if (col > w && col < words) {                           // the kept rows into the words after this block, loads in flight together
                unsigned long long m = keep;
                while (m) {
                    unsigned long long r[4];
                    int b = 0;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {                   // four rows per trip; the last row again when fewer are left
                        b = m ? __ffsll((long long)m) - 1 : b;
                        m &= m - 1ull;
                        r[p] = mat[(long long)(w * 64 + b) * pitch + col];
                    }
                    rem[q] |= (r[0] | r[1]) | (r[2] | r[3]);
                }
            }
        }
    }
    return min(kept, limit);
}
