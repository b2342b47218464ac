// Detectron2's ROIPooler (modeling/poolers.py) with ROIAlignV2 = torchvision's roi_align(aligned=True) on the device: the level of every
// box, the pooled features of all levels and images in one launch, and the gradient of the feature maps without float atomics.
// Written from the two published definitions; the reference builds the pooler at custom_cascade_rcnn.py:117-122 and
// roi_heads.py:674-679, 709-716 and calls it at custom_cascade_rcnn.py:326.
//
//   rp_prepare_kernel   one thread per box: info[r] = (image, level), (-1, 0) for a box the device refuses.  The image is the last
//                       entry of `first` (the prefix sums of the boxes per image) that is <= r, or column 0 of a [R,5] roi; the level is
//                       Detectron2's assign_boxes_to_levels in float32, operation by operation:
//                         s = sqrt((x2 - x1) * (y2 - y1));  t = s / canonical_box_size + 1e-8f;  v = floor(canonical_level + log2(t))
//                         level = clamp(v, min_level, max_level) - min_level            (a NaN v, from a negative area, gives min_level)
//   rp_forward_kernel   one workgroup of 256 threads per box (per box and chunk of >= 32 channels when the boxes are few).  ROIAlign is separable: per box
//                         out[c] = Ay F[c] Ax^T / count,   Ay[ph, y] = the summed weight of row y over the samples of bin ph,
//                       so the workgroup lays the two axis tables into LDS once (rp_tables) and every channel of its chunk reuses them; a
//                       thread owns a bin (ph, pw), pw fastest, walks the channels and adds  sum_y Ay[ph,y] * (sum_x Ax[pw,x] * F[c,y,x]).
//   rp_backward_kernel  the owner form: a workgroup owns (level, image, tile of 8 x 32 pixels, chunk of 32 channels), a thread one
//                       pixel of the tile and its 32 channels in registers.  It walks the image's boxes in index order, 256 at a time:
//                       the boxes of its level whose tap extent (a conservative one, from the box alone) meets the tile are compacted
//                       in index order (ballot + prefix), and for each the box's 32 x P x P output gradients are staged in LDS in one
//                       coalesced pass (P <= 16; read in place above that), the tables are rebuilt and
//                         grad[c,y,x] += sum_ph sum_pw ((Ay[ph,y] * Ax[pw,x]) / count_r) * g[r,c,ph,pw],  ph outer, pw inner.
//                       The tile is written with plain stores, zeros included: no memset, no atomics, the order of every sum is fixed by
//                       the indices, so the same input gives the same bytes on every run.
//
// The axis tables (rp_tables).  float32, no contraction, torchvision's operations:
//   start = lo * scale - .5f;  roi = (hi * scale - .5f) - start;  bin = roi / P;  grid = sampling_ratio > 0 ? sampling_ratio : ceil(bin)
//   coordinate(p, i) = start + p * bin + (i + .5f) * bin / grid;  outside [-1, size]: the sample adds 0.  Else c <= 0 -> 0; low = (int)c;
//   low >= size - 1 -> low = high = size - 1, c = low; else high = low + 1;  l = c - low adds to tap `high`, h = 1 - l to tap `low`.
// The coordinate does not decrease with i (a chain of monotone roundings), so the samples of a bin inside [-1, size] are one run, found
// by bisection on the float32 expression itself (roi_align_axis.h, shared with mask_loss.hip), and their taps are the contiguous rows
// [tap_lo, tap_lo + n).  One thread walks one bin's run in sample order with the two open taps in registers, so Ay[ph, y] is the sum of
// its weights in sample order.  The tables are compact: bin after bin, n weights each; neighbouring bins share at most a few rows, so an
// axis takes at most size + 4 P + 8 floats whatever the box and whatever the grid -- both are walked by loops, neither is capped.
// Should the runs not fit (the bound rules it out) the box is treated as a refused one, never written past the table.
//
// What the device refuses (a zero row, no gradient): an image or level index out of range, a level without a map, a coordinate that is
// not finite or beyond +-2^20.  roi <= 0 on an axis: zeros too (torchvision would average an empty grid).  A tap whose summed weight is
// exactly 0 adds 0 whatever the map holds there.
#pragma clang fp contract(off)
#include "umr_common.h"
#include "roi_align_axis.h"
#include <algorithm>
#include <string.h>

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_MAX_LEVELS = 8;
constexpr int RP_MAX_P = 64;
constexpr int RP_CH = 32;                            // channels per workgroup in the backward, the least in the forward
constexpr int RP_FWD_CH = 4;                         // channels a forward thread sums side by side
constexpr int RP_TILE_H = 8, RP_TILE_W = 32;         // the backward's tile: one pixel per thread
constexpr float RP_MAX_COORD = 1048576.f;            // 2^20
constexpr float RP_MAX_SCALE = 16.f;                 // roi <= 2^25: the grid is an int with room to spare
constexpr int64_t RP_MAX_LDS = 64 * 1024;

static_assert(RP_TILE_H * RP_TILE_W == RP_THREADS, "one pixel per thread");

struct RpLevel {
    void* f;                 // features (forward) or their gradient (backward), [N,C,H,W]
    int H, W;
    float scale;
    int tiles_x, tiles;      // backward: tiles per row, tiles per image
    int64_t tile_first;      // backward: the level's first workgroup
};
struct RpLevels {            // passed to the kernels by value: no table upload
    RpLevel l[RP_MAX_LEVELS];
    int n;
};

__device__ __forceinline__ RpLevel rp_pick(const RpLevels& lv, int l) {
    RpLevel r = lv.l[0];
#pragma unroll
    for (int k = 1; k < RP_MAX_LEVELS; ++k)
        if (l == k) r = lv.l[k];
    return r;
}

__host__ __device__ inline int rp_cap(int size, int P) { return size + 4 * P + 8; }
__host__ __device__ inline int rp_meta_ints(int P) { return 8 * P + 2 + RP_THREADS + 4; }   // runs, tap rows, offsets; the backward's list
inline int64_t rp_lds_bytes(int P, int max_h, int max_w) { return 4 * ((int64_t)rp_meta_ints(P) + rp_cap(max_h, P) + rp_cap(max_w, P)); }

struct RpGeom {
    float start_h, start_w, bin_h, bin_w, count;
    int grid_h, grid_w;
    bool sampled;
};

__device__ __forceinline__ bool rp_coords_ok(float x1, float y1, float x2, float y2) {      // NaN fails
    return fabsf(x1) <= RP_MAX_COORD && fabsf(y1) <= RP_MAX_COORD && fabsf(x2) <= RP_MAX_COORD && fabsf(y2) <= RP_MAX_COORD;
}

__device__ __forceinline__ RpGeom rp_geom(float x1, float y1, float x2, float y2, float scale, int P, int sampling_ratio, bool ok) {
    RpGeom g;
    g.start_w = x1 * scale - .5f;
    g.start_h = y1 * scale - .5f;
    const float roi_w = (x2 * scale - .5f) - g.start_w, roi_h = (y2 * scale - .5f) - g.start_h;
    g.bin_w = __fdiv_rn(roi_w, (float)P);
    g.bin_h = __fdiv_rn(roi_h, (float)P);
    g.sampled = ok && roi_w > 0.f && roi_h > 0.f;
    g.grid_w = !g.sampled ? 0 : sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.bin_w);
    g.grid_h = !g.sampled ? 0 : sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.bin_h);
    g.sampled = g.sampled && g.grid_w > 0 && g.grid_h > 0;              // a denormal roi: the reference's loops are empty too
    g.count = fmaxf((float)((long long)g.grid_h * g.grid_w), 1.f);
    return g;
}

// views of the axis tables in LDS: index k = axis * P + p, axis 0 = rows against H, 1 = columns against W
struct RpTables {
    int* run_a;      // [2P] first sample of the bin's run
    int* run_n;      // [2P] samples in the run
    int* tap_lo;     // [2P] the bin's first tap
    int* off;        // [2][P + 1] where the bin's weights start in its axis' table
    float* ent_h;    // [cap_h]
    float* ent_w;    // [cap_w]
};

__device__ __forceinline__ RpTables rp_views(int* smem, int P, int max_h) {
    RpTables t;
    t.run_a = smem;
    t.run_n = smem + 2 * P;
    t.tap_lo = smem + 4 * P;
    t.off = smem + 6 * P;
    t.ent_h = (float*)(smem + rp_meta_ints(P));
    t.ent_w = t.ent_h + rp_cap(max_h, P);
    return t;
}

// Lays both tables of one box; every thread of the workgroup calls it with the same arguments.  false: the runs do not fit.
__device__ bool rp_tables(const RpTables& t, const RpGeom& g, int P, int H, int W, int cap_h, int cap_w) {
    const int tid = threadIdx.x;
    __syncthreads();                                                    // whoever still reads the previous box's tables
    for (int k = tid; k < 2 * P; k += RP_THREADS) {
        const int axis = k >= P, p = k - axis * P;
        const float start = axis ? g.start_w : g.start_h, bin = axis ? g.bin_w : g.bin_h;
        const int grid = axis ? g.grid_w : g.grid_h, size = axis ? W : H;
        const int a = roi_axis_first(start, bin, grid, p, -1.f, false);
        const int b = max(a, roi_axis_first(start, bin, grid, p, (float)size, true));
        int lo = 0, n = 0;
        if (b > a) {
            const int2 e0 = roi_axis_entry(roi_axis_coord(start, bin, grid, p, a), size);
            const int2 e1 = roi_axis_entry(roi_axis_coord(start, bin, grid, p, b - 1), size);
            if (e0.x >= 0 && e1.x >= e0.x) {
                lo = e0.x;
                n = e1.x + (e1.x < size - 1 ? 1 : 0) - lo + 1;
            }
        }
        t.run_a[k] = a;
        t.run_n[k] = n > 0 ? b - a : 0;
        t.tap_lo[k] = lo;
        t.off[axis * (P + 1) + p + 1] = n;
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {                                        // two waves, one axis each
        int* off = t.off + (tid ? P + 1 : 0);
        off[0] = 0;
        for (int p = 0; p < P; ++p) off[p + 1] += off[p];
    }
    __syncthreads();
    const int tot_h = t.off[P], tot_w = t.off[2 * P + 1];
    if (tot_h > cap_h || tot_w > cap_w) return false;                   // workgroup-uniform
    for (int k = tid; k < tot_h; k += RP_THREADS) t.ent_h[k] = 0.f;
    for (int k = tid; k < tot_w; k += RP_THREADS) t.ent_w[k] = 0.f;
    __syncthreads();
    for (int k = tid; k < 2 * P; k += RP_THREADS) {
        const int axis = k >= P, p = k - axis * P;
        const float start = axis ? g.start_w : g.start_h, bin = axis ? g.bin_w : g.bin_h;
        const int grid = axis ? g.grid_w : g.grid_h, size = axis ? W : H;
        const int a = t.run_a[k], cnt = t.run_n[k], lo = t.tap_lo[k];
        const int n = t.off[axis * (P + 1) + p + 1] - t.off[axis * (P + 1) + p];
        float* ent = (axis ? t.ent_w : t.ent_h) + t.off[axis * (P + 1) + p];
        int cur = -1;
        float a0 = 0.f, a1 = 0.f;                                       // the sums of taps cur and cur + 1
        auto put = [&](int tap, float v) {
            const int j = tap - lo;
            if (j >= 0 && j < n) ent[j] = v;
        };
        for (int i = a; i < a + cnt; ++i) {
            const int2 e = roi_axis_entry(roi_axis_coord(start, bin, grid, p, i), size);
            if (e.x < 0) continue;
            const float l = __int_as_float(e.y), h = 1.f - l;
            if (e.x != cur) {
                if (cur >= 0) {
                    put(cur, a0);
                    if (e.x == cur + 1) {
                        a0 = a1;
                    } else {
                        put(cur + 1, a1);
                        a0 = 0.f;
                    }
                    a1 = 0.f;
                }
                cur = e.x;
            }
            a0 += h;
            a1 += l;
        }
        if (cur >= 0) {
            put(cur, a0);
            put(cur + 1, a1);
        }
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(RP_THREADS) void rp_prepare_kernel(const float* __restrict__ boxes, int box_stride, int R,
                                                                const int32_t* __restrict__ first, int N, int assign, int min_level,
                                                                int max_level, float canonical_size, float canonical_level,
                                                                int2* __restrict__ info) {
    const int r = blockIdx.x * RP_THREADS + threadIdx.x;
    if (r >= R) return;
    const float* b = boxes + (int64_t)r * box_stride + (box_stride - 4);
    const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    bool ok = rp_coords_ok(x1, y1, x2, y2);
    int image = 0;
    if (first) {
        int lo = 0, hi = N;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= r) lo = mid; else hi = mid;
        }
        image = lo;
        ok = ok && first[lo] <= r && r < first[lo + 1];
    } else {
        const float f = boxes[(int64_t)r * box_stride];
        ok = ok && f >= 0.f && f < (float)N && f == floorf(f);
        image = ok ? (int)f : 0;
    }
    int level = 0;
    if (assign && ok) {
        const float s = __fsqrt_rn((x2 - x1) * (y2 - y1));
        const float t = __fdiv_rn(s, canonical_size) + 1e-8f;
        float v = floorf(canonical_level + log2f(t));
        v = v >= (float)min_level ? v : (float)min_level;               // NaN -> min_level
        v = v <= (float)max_level ? v : (float)max_level;
        level = (int)v - min_level;
    }
    info[r] = ok ? make_int2(image, level) : make_int2(-1, 0);
}

template <typename T>
__global__ __launch_bounds__(RP_THREADS) void rp_forward_kernel(RpLevels lv, int N, int C, const float* __restrict__ boxes, int box_stride,
                                                                const int2* __restrict__ info, int P, int sampling_ratio, int max_h,
                                                                int max_w, int ch_per, T* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int rp_smem[];
    const RpTables t = rp_views(rp_smem, P, max_h);
    const int tid = threadIdx.x, r = blockIdx.x, c0 = blockIdx.y * ch_per, nc = min(ch_per, C - c0), PP = P * P;
    const int2 inf = info[r];
    bool ok = inf.x >= 0 && inf.x < N && inf.y >= 0 && inf.y < lv.n;
    const RpLevel L = rp_pick(lv, ok ? inf.y : 0);
    const int H = L.H, W = L.W;
    ok = ok && L.f && H > 0 && W > 0 && H <= max_h && W <= max_w;
    const float* b = boxes + (int64_t)r * box_stride + (box_stride - 4);
    const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    ok = ok && rp_coords_ok(x1, y1, x2, y2);
    const RpGeom g = rp_geom(x1, y1, x2, y2, L.scale, P, sampling_ratio, ok);
    bool sampled = g.sampled;
    if (sampled) sampled = rp_tables(t, g, P, H, W, rp_cap(max_h, P), rp_cap(max_w, P));      // workgroup-uniform
    const int* off_h = t.off;
    const int* off_w = t.off + P + 1;
    const int64_t plane = (int64_t)H * W;
    const T* f0 = (const T*)L.f + ((int64_t)(ok ? inf.x : 0) * C + c0) * plane;
    T* o0 = out + ((int64_t)r * C + c0) * PP;
    if (!sampled) {                                                     // workgroup-uniform
        for (int e = tid; e < nc * PP; e += RP_THREADS) o0[e] = from_f32<T>(0.f);
        return;
    }
    // a thread keeps its bin and walks the channels: the bin's runs are read once, consecutive lanes read consecutive bins of one channel
    const int lane_bins = min(PP, RP_THREADS), groups = RP_THREADS / lane_bins, cg = tid / lane_bins;
    for (int bin = tid % lane_bins; cg < groups && bin < PP; bin += lane_bins) {
        const int ph = bin / P, pw = bin - ph * P;
        const int ya = off_h[ph], yn = off_h[ph + 1] - ya, y_lo = t.tap_lo[ph];
        const int xa = off_w[pw], xn = off_w[pw + 1] - xa, x_lo = t.tap_lo[P + pw];
        for (int c = cg; c < nc; c += RP_FWD_CH * groups) {                 // RP_FWD_CH channels at once: their loads are in flight together
            float acc[RP_FWD_CH];
#pragma unroll
            for (int u = 0; u < RP_FWD_CH; ++u) acc[u] = 0.f;
            for (int j = 0; j < yn; ++j) {
                const float wy = t.ent_h[ya + j];
                const int64_t row = (int64_t)min(max(y_lo + j, 0), H - 1) * W;          // the tables hold taps of the map only; held to it anyway
                float racc[RP_FWD_CH];
#pragma unroll
                for (int u = 0; u < RP_FWD_CH; ++u) racc[u] = 0.f;
                for (int i = 0; i < xn; ++i) {
                    const float wx = t.ent_w[xa + i];
                    const T* tap = f0 + row + min(max(x_lo + i, 0), W - 1);
#pragma unroll
                    for (int u = 0; u < RP_FWD_CH; ++u) {
                        const int cu = c + u * groups;
                        const float v = cu < nc ? to_f32<T>(tap[(int64_t)cu * plane]) : 0.f;
                        racc[u] += wx == 0.f ? 0.f : wx * v;             // a tap of weight 0 adds 0 whatever it holds
                    }
                }
#pragma unroll
                for (int u = 0; u < RP_FWD_CH; ++u) acc[u] += wy == 0.f ? 0.f : wy * racc[u];
            }
#pragma unroll
            for (int u = 0; u < RP_FWD_CH; ++u) {
                const int cu = c + u * groups;
                if (cu < nc) o0[(int64_t)cu * PP + bin] = from_f32<T>(__fdiv_rn(acc[u], g.count));
            }
        }
    }
}

// STAGED: the box's output gradient goes through LDS.  32 running sums per thread: held to 128 registers, four workgroups per CU, so
// that one workgroup's table building (a few lanes of one wave) overlaps the others' sums.
template <typename T, bool STAGED>
__global__ __launch_bounds__(RP_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void rp_backward_kernel(
    RpLevels lv, int N, int C, const float* __restrict__ boxes, int box_stride, const int2* __restrict__ info,
    const int32_t* __restrict__ first, int R, int P, int sampling_ratio, int max_h, int max_w, const T* __restrict__ gout) {
    extern __shared__ __attribute__((aligned(16))) int rp_smem[];
    const RpTables t = rp_views(rp_smem, P, max_h);
    int* list = rp_smem + 8 * P + 2;                                    // [256] the batch's boxes that meet the tile, in index order
    int* wcnt = list + RP_THREADS;                                      // [4]
    float* gs = t.ent_w + rp_cap(max_w, P);                             // [32][P][P] the box's output gradient, when STAGED
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, PP = P * P;
    const int c0 = blockIdx.y * RP_CH, nc = min(RP_CH, C - c0);

    // ---- what this workgroup owns
    int l = -1;
#pragma unroll
    for (int k = 0; k < RP_MAX_LEVELS; ++k)
        if (k < lv.n && (int64_t)blockIdx.x >= lv.l[k].tile_first && (int64_t)blockIdx.x < lv.l[k].tile_first + (int64_t)N * lv.l[k].tiles) l = k;
    if (l < 0) return;                                                  // workgroup-uniform; the grid is the sum of the levels' tiles
    const RpLevel L = rp_pick(lv, l);
    const int H = L.H, W = L.W;
    const int64_t local = (int64_t)blockIdx.x - L.tile_first;
    const int n = (int)(local / L.tiles), tile = (int)(local - (int64_t)n * L.tiles);
    const int ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
    const int y0 = ty * RP_TILE_H, x0 = tx * RP_TILE_W, y1t = min(y0 + RP_TILE_H, H) - 1, x1t = min(x0 + RP_TILE_W, W) - 1;
    const int y = y0 + tid / RP_TILE_W, x = x0 + tid % RP_TILE_W;
    const bool inside = y < H && x < W;

    float acc[RP_CH];
#pragma unroll
    for (int c = 0; c < RP_CH; ++c) acc[c] = 0.f;

    int r_begin = 0, r_end = R;
    if (first) {                                                        // the pooler's boxes are in image order
        r_begin = max(first[n], 0);
        r_end = min(first[n + 1], R);
    }
    for (int base = r_begin; base < r_end; base += RP_THREADS) {
        const int row = base + tid;
        bool hit = false;
        if (row < r_end) {
            const int2 inf = info[row];
            if (inf.x == n && inf.y == l) {
                const float* b = boxes + (int64_t)row * box_stride + (box_stride - 4);
                const float bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
                if (rp_coords_ok(bx1, by1, bx2, by2)) {
                    // every tap of a sample lies within one pixel of [start, start + roi]; the float32 coordinate is off by a few ulps
                    // of the largest term (|start| + roi): one more pixel plus 2^-20 of that covers it.  Only a filter: the tables decide.
                    const float sw = bx1 * L.scale - .5f, sh = by1 * L.scale - .5f;
                    const float ew = bx2 * L.scale - .5f, eh = by2 * L.scale - .5f;
                    const float kw = 2.f + (fabsf(sw) + fabsf(ew)) * 9.5367431640625e-7f, kh = 2.f + (fabsf(sh) + fabsf(eh)) * 9.5367431640625e-7f;
                    hit = ew > sw && eh > sh && floorf(sh) - kh <= (float)y1t && ceilf(eh) + kh >= (float)y0 &&
                          floorf(sw) - kw <= (float)x1t && ceilf(ew) + kw >= (float)x0;
                }
            }
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wcnt[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < RP_THREADS / 64; ++k) {
            before += k < wv ? wcnt[k] : 0;
            total += wcnt[k];
        }
        if (hit) list[before + __popcll(m & ((1ull << lane) - 1ull))] = row;
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const int rr = list[k];
            const float* b = boxes + (int64_t)rr * box_stride + (box_stride - 4);
            const RpGeom g = rp_geom(b[0], b[1], b[2], b[3], L.scale, P, sampling_ratio, true);
            if (!g.sampled) continue;                                   // workgroup-uniform
            const T* g0 = gout + ((int64_t)rr * C + c0) * PP;
            if constexpr (STAGED) {                                     // one coalesced pass instead of a gather per pixel
                __syncthreads();                                        // whoever still reads the previous box's gradient
                for (int i = tid; i < nc * PP; i += RP_THREADS) gs[i] = to_f32<T>(g0[i]);
            }
            if (!rp_tables(t, g, P, H, W, rp_cap(max_h, P), rp_cap(max_w, P))) continue;
            if (inside) {
                // the bins whose taps include this pixel: one range per axis (the tap rows do not decrease with the bin)
                int ph_a = P, ph_b = -1, pw_a = P, pw_b = -1;
                for (int p = 0; p < P; ++p) {
                    const int jy = y - t.tap_lo[p], jx = x - t.tap_lo[P + p];
                    if (jy >= 0 && jy < t.off[p + 1] - t.off[p]) { ph_a = min(ph_a, p); ph_b = p; }
                    if (jx >= 0 && jx < t.off[P + 2 + p] - t.off[P + 1 + p]) { pw_a = min(pw_a, p); pw_b = p; }
                }
                if (ph_b < 0 || pw_b < 0) continue;                     // no barrier follows before the next box's own
                for (int ph = ph_a; ph <= ph_b; ++ph) {
                    const int jy = y - t.tap_lo[ph], ya = t.off[ph];
                    if (jy < 0 || jy >= t.off[ph + 1] - ya) continue;
                    const float wy = t.ent_h[ya + jy];
                    if (wy == 0.f) continue;
                    for (int pw = pw_a; pw <= pw_b; ++pw) {
                        const int jx = x - t.tap_lo[P + pw], xa = t.off[P + 1 + pw];
                        if (jx < 0 || jx >= t.off[P + 2 + pw] - xa) continue;
                        const float wx = t.ent_w[xa + jx];
                        if (wx == 0.f) continue;
                        const float w = __fdiv_rn(wy * wx, g.count);
                        if constexpr (STAGED) {
                            const float* gp = gs + ph * P + pw;
#pragma unroll
                            for (int c = 0; c < RP_CH; ++c)
                                if (c < nc) acc[c] += w * gp[c * PP];
                        } else {
                            const T* gp = g0 + ph * P + pw;
#pragma unroll
                            for (int c = 0; c < RP_CH; ++c)
                                if (c < nc) acc[c] += w * to_f32<T>(gp[(int64_t)c * PP]);
                        }
                    }
                }
            }
        }
        __syncthreads();                                                // list and wcnt are rewritten by the next batch
    }
    if (inside) {
        T* o = (T*)L.f + (((int64_t)n * C + c0) * H + y) * W + x;
        const int64_t plane = (int64_t)H * W;
#pragma unroll
        for (int c = 0; c < RP_CH; ++c)
            if (c < nc) o[(int64_t)c * plane] = from_f32<T>(acc[c]);
    }
}

// levels: 4 int64 per level -- pointer, H, W, the bits of the float scale (include/umr.h)
int rp_read_levels(const int64_t* levels, int n_levels, int64_t N, bool backward, RpLevels* lv, int* max_h, int* max_w, int64_t* tiles) {
    UMR_CHECK_ARG(levels && n_levels >= 1 && n_levels <= RP_MAX_LEVELS, "roi_pool: 1 to 8 levels");
    memset(lv, 0, sizeof(*lv));
    lv->n = n_levels;
    *max_h = *max_w = 1;
    *tiles = 0;
    for (int k = 0; k < n_levels; ++k) {
        RpLevel& L = lv->l[k];
        const int64_t H = levels[4 * k + 1], W = levels[4 * k + 2];
        const uint32_t bits = (uint32_t)levels[4 * k + 3];
        memcpy(&L.scale, &bits, 4);
        L.f = (void*)(uintptr_t)levels[4 * k];
        UMR_CHECK_ARG(H >= 1 && W >= 1 && H * W < ((int64_t)1 << 31), "roi_pool: a map must have H, W >= 1 and fewer than 2^31 pixels");
        UMR_CHECK_ARG(L.scale > 0.f && L.scale <= RP_MAX_SCALE, "roi_pool: a scale must be in (0, 16]");
        UMR_CHECK_ARG(backward || L.f, "roi_pool: null feature map");
        L.H = (int)H;
        L.W = (int)W;
        *max_h = std::max(*max_h, L.H);
        *max_w = std::max(*max_w, L.W);
        L.tiles_x = (L.W + RP_TILE_W - 1) / RP_TILE_W;
        L.tiles = L.f ? L.tiles_x * ((L.H + RP_TILE_H - 1) / RP_TILE_H) : 0;      // backward: a level without a gradient buffer is skipped
        L.tile_first = *tiles;
        *tiles += N * L.tiles;
    }
    return UMR_OK;
}

int rp_check_common(int64_t N, int C, int dtype, const float* boxes, int box_stride, const int32_t* info, int64_t R, int P,
                    int sampling_ratio, int max_h, int max_w) {
    UMR_CHECK_ARG(N >= 1 && N <= INT_MAX && C >= 1 && C <= 65535 * RP_CH, "roi_pool: N >= 1, 1 <= C <= 65535 * 32");
    UMR_CHECK_ARG(dtype == UMR_F32 || dtype == UMR_BF16, "roi_pool: features must be UMR_F32 or UMR_BF16");
    UMR_CHECK_ARG(R >= 0 && R <= INT_MAX, "roi_pool: 0 to 2^31 - 1 boxes");
    UMR_CHECK_ARG(box_stride == 4 || box_stride == 5, "roi_pool: boxes are [R,4] or [R,5] rows");
    UMR_CHECK_ARG(R == 0 || (boxes && info), "roi_pool: null boxes or info");
    UMR_CHECK_ARG(P >= 1 && P <= RP_MAX_P, "roi_pool: the output side must be in [1, 64]");
    UMR_CHECK_ARG(sampling_ratio >= 0 && sampling_ratio <= 1024, "roi_pool: the sampling ratio must be in [0, 1024]");
    UMR_CHECK_ARG(rp_lds_bytes(P, max_h, max_w) <= RP_MAX_LDS, "roi_pool: the axis tables of a map this large do not fit the LDS (4 * (H + W) + 64 * P + 1112 bytes <= 64 KiB)");
    return UMR_OK;
}

}  // namespace

extern "C" int umr_roi_pool_prepare(const float* boxes, int box_stride, int64_t R, const int32_t* first, int64_t N, int n_levels,
                                    int min_level, int max_level, float canonical_box_size, int canonical_level, int32_t* info,
                                    umr_stream_t stream) {
    UMR_CHECK_ARG(R >= 0 && R <= INT_MAX && N >= 1 && N <= INT_MAX, "roi_pool: 0 to 2^31 - 1 boxes, at least one image");
    UMR_CHECK_ARG(box_stride == 4 || box_stride == 5, "roi_pool: boxes are [R,4] or [R,5] rows");
    UMR_CHECK_ARG((box_stride == 5) == (first == nullptr), "roi_pool: [R,4] boxes come with `first`, [R,5] rois carry their image");
    UMR_CHECK_ARG(n_levels >= 1 && n_levels <= RP_MAX_LEVELS && max_level - min_level + 1 == n_levels, "roi_pool: 1 to 8 levels, min_level to max_level");
    UMR_CHECK_ARG(canonical_box_size > 0.f, "roi_pool: canonical_box_size must be positive");
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(boxes && info, "roi_pool: null boxes or info");
    rp_prepare_kernel<<<(unsigned)((R + RP_THREADS - 1) / RP_THREADS), RP_THREADS, 0, (hipStream_t)stream>>>(
        boxes, box_stride, (int)R, first, (int)N, n_levels > 1, min_level, max_level, canonical_box_size, (float)canonical_level, (int2*)info);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_roi_pool_forward(const int64_t* levels, int n_levels, int64_t N, int C, int dtype, const float* boxes, int box_stride,
                                    const int32_t* info, int64_t R, int P, int sampling_ratio, void* out, umr_stream_t stream) {
    RpLevels lv;
    int max_h, max_w;
    int64_t tiles;
    if (int st = rp_read_levels(levels, n_levels, N, false, &lv, &max_h, &max_w, &tiles)) return st;
    if (int st = rp_check_common(N, C, dtype, boxes, box_stride, info, R, P, sampling_ratio, max_h, max_w)) return st;
    if (R == 0) return UMR_OK;
    UMR_CHECK_ARG(out, "roi_pool: null output");
    // the tables are laid once per workgroup: with boxes enough to fill the chip one workgroup takes all channels of its box, with few
    // boxes the channels are shared out in chunks of at least 32
    const int chunks = (int)std::min<int64_t>((C + RP_CH - 1) / RP_CH, std::max<int64_t>(1, (2048 + R - 1) / R));
    const int ch_per = (C + chunks - 1) / chunks;
    const dim3 grid((unsigned)R, (unsigned)((C + ch_per - 1) / ch_per));
    const int lds = (int)rp_lds_bytes(P, max_h, max_w);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == UMR_F32)
        rp_forward_kernel<float><<<grid, RP_THREADS, lds, s>>>(lv, (int)N, C, boxes, box_stride, (const int2*)info, P, sampling_ratio, max_h, max_w, ch_per, (float*)out);
    else
        rp_forward_kernel<bf16_t><<<grid, RP_THREADS, lds, s>>>(lv, (int)N, C, boxes, box_stride, (const int2*)info, P, sampling_ratio, max_h, max_w, ch_per, (bf16_t*)out);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int umr_roi_pool_backward(const int64_t* levels, int n_levels, int64_t N, int C, int dtype, const float* boxes, int box_stride,
                                     const int32_t* info, const int32_t* first, int64_t R, int P, int sampling_ratio, const void* grad_out,
                                     umr_stream_t stream) {
    RpLevels lv;
    int max_h, max_w;
    int64_t tiles;
    if (int st = rp_read_levels(levels, n_levels, N, true, &lv, &max_h, &max_w, &tiles)) return st;
    if (int st = rp_check_common(N, C, dtype, boxes, box_stride, info, R, P, sampling_ratio, max_h, max_w)) return st;
    UMR_CHECK_ARG(R == 0 || grad_out, "roi_pool: null output gradient");
    UMR_CHECK_ARG(tiles <= INT_MAX, "roi_pool: more than 2^31 - 1 tiles");
    if (tiles == 0) return UMR_OK;
    const dim3 grid((unsigned)tiles, (unsigned)((C + RP_CH - 1) / RP_CH));
    // the box's output gradient is staged in LDS, [32][P][P] floats, when that fits beside the tables (P <= 16 on the recipe's maps)
    const int64_t stage_bytes = 4 * (int64_t)RP_CH * P * P;
    const int staged = stage_bytes <= 32 * 1024 && rp_lds_bytes(P, max_h, max_w) + stage_bytes <= RP_MAX_LDS;
    const int lds = (int)(rp_lds_bytes(P, max_h, max_w) + (staged ? stage_bytes : 0));
    hipStream_t s = (hipStream_t)stream;
#define RP_BACKWARD(T, STAGED)                                                                                                             \
    rp_backward_kernel<T, STAGED><<<grid, RP_THREADS, lds, s>>>(lv, (int)N, C, boxes, box_stride, (const int2*)info, first, (int)R, P,     \
                                                                sampling_ratio, max_h, max_w, (const T*)grad_out)
    if (dtype == UMR_F32) {
        if (staged) RP_BACKWARD(float, true); else RP_BACKWARD(float, false);
    } else {
        if (staged) RP_BACKWARD(bf16_t, true); else RP_BACKWARD(bf16_t, false);
    }
#undef RP_BACKWARD
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
