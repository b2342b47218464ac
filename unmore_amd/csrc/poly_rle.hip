// COCO run-length records of POLYGON segmentations on the device: pycocotools' annToRLE for polygons (maskApi.c rleFrPoly per polygon,
// then rleMerge = union over an annotation's polygons), so that polygon ground truths enter the evaluator (coco_eval.hip) as the
// run-length strings everything downstream already takes.  The arithmetic is the one unmore_amd/rle.py restates sequentially
// (polygon_points_numpy / polygon_crossings_numpy / from_polygons_numpy); the device is compared with it byte for byte.
//
// Vertices are scaled by 5 and truncated; every edge is a run of max(dx,dy)+1 points on that fine grid; wherever two consecutive
// points of the concatenated outline differ in u, and the step is over the centre line of a pixel column xd inside the image, a
// CROSSING a = xd*H + yd is recorded (yd: the row of the upper point, clamped to [0,H], rounded up).  Pixel p = x*H + y is set iff
// an odd number of the polygon's crossings are <= p; an annotation's mask is the OR of its polygons' masks.
//
// Three kernels, 256 threads, no atomics, no waiting between workgroups; the same input gives the same bytes on every run:
//   poly_generate_kernel, one workgroup per polygon: the integer vertices; the edges' point counts prefix-summed (int64: one edge
//     can hold 10^7 points) into the polygon's table; then one thread per point j >= 1 of the outline: the edge of j by bisecting that
//     table, points j and j-1 both in closed form (no dependence between threads), the crossing test; survivors are compacted by
//     ballot rank, in outline order, into the polygon's slice of the crossing list (its capacity is the host's bound: an edge
//     crosses every column at most once, so min(dx, W) + 1 per edge).
//   poly_sort_kernel, one workgroup per annotation: every polygon's list sorted in place; for several polygons the lists are then
//     copied one after the other into the annotation's candidate slice and that is sorted too (one polygon: its own list is the
//     candidate list).  The sort is a bitonic network whose every compare-exchange puts the smaller key at the smaller index, which
//     makes a missing partner (index >= n) the same as a key of +infinity: any n, no padding.  Up to POLY_LDS_KEYS keys it runs in
//     LDS, beyond that in the list's own slice in memory, with the same steps and a barrier after each.  Also the number of
//     candidates below H*W (a crossing can equal H*W: the end of the image, not a pixel).
//   poly_chars_kernel (measure pass / write pass), one workgroup per annotation: the back end of rle_stream.h over the candidates
//     below H*W.  value(p) = the union's state at pixel cand[p]: for each polygon the parity of its count of crossings <= cand[p], by
//     bisection of its sorted list; gpos(p) = cand[p]; the pixel before the stream is 0.  Between two candidates no polygon's parity
//     changes, so the boundaries of the union's runs are exactly the candidates whose value differs from the previous candidate's;
//     equal candidates have equal values and cannot flag twice.
//
// Contraction is off for the whole file: ys + s*t fused into one rounding is an ulp away from C's two and decides the .5 ties of the
// truncation.  The divisions by dx, dy and 5.0 are IEEE divisions (the library is built without fast-math flags).
#pragma clang fp contract(off)
#include "umr_common.h"
#include "rle_stream.h"

namespace {

constexpr int POLY_THREADS = RLE_THREADS;          // the back end's workgroup
constexpr int POLY_LDS_KEYS = 4096;                // 16 KiB: the bitonic sort's LDS capacity, in keys

struct PolyTables {
    const double* xy;                  // [2 * V]
    const int64_t* poly_off;           // [NP + 1], in vertices
    const int64_t* ann_poly;           // [NA + 1], in polygons
    const int64_t* ann_size;           // [NA][2] = H, W
    const int64_t* cross_off;          // [NP + 1]: the polygons' slices of the crossing list
    int64_t V, C;
    int NP, NA;
};
struct PolyWork {
    int32_t* vxy;                      // [2 * V] integer vertices, x then y per vertex
    int64_t* eoff;                     // [V + NP]: polygon q's edge table at poly_off[q] + q, k + 1 entries
    int32_t* cnt;                      // [NP] crossings found
    int32_t* ncand;                    // [NA][2]: candidates, candidates below H*W
    uint32_t* cross;                   // [C]
    uint32_t* cand;                    // [C]
};

// polygon q's vertex range and crossing slice, checked against the extents: k = 0 when the tables are inconsistent
struct PolyRange {
    int64_t v0, c0;
    int k, cap;
};
__device__ __forceinline__ PolyRange poly_range(const PolyTables& t, int q) {
    PolyRange r;
    const int64_t v0 = t.poly_off[q], v1 = t.poly_off[q + 1], c0 = t.cross_off[q], c1 = t.cross_off[q + 1];
    const bool ok = v0 >= 0 && v1 > v0 && v1 <= t.V && v1 - v0 < ((int64_t)1 << 30) && c0 >= 0 && c1 >= c0 && c1 <= t.C && c1 - c0 < ((int64_t)1 << 31);
    r.v0 = ok ? v0 : 0; r.c0 = ok ? c0 : 0;
    r.k = ok ? (int)(v1 - v0) : 0; r.cap = ok ? (int)(c1 - c0) : 0;
    return r;
}
struct AnnRange {
    int q0, q1;                        // polygons
    uint32_t H, W, HW;
    bool ok;
};
__device__ __forceinline__ AnnRange ann_range(const PolyTables& t, int a) {
    AnnRange r;
    const int64_t q0 = t.ann_poly[a], q1 = t.ann_poly[a + 1], H = t.ann_size[a * 2], W = t.ann_size[a * 2 + 1];
    r.ok = q0 >= 0 && q1 >= q0 && q1 <= t.NP && H > 0 && W > 0 && H < ((int64_t)1 << 31) && W < ((int64_t)1 << 31) && H * W < ((int64_t)1 << 31);
    r.q0 = r.ok ? (int)q0 : 0; r.q1 = r.ok ? (int)q1 : 0;
    r.H = r.ok ? (uint32_t)H : 1u; r.W = r.ok ? (uint32_t)W : 1u; r.HW = r.H * r.W;
    return r;
}
// the annotation of polygon q: the last a with ann_poly[a] <= q
__device__ __forceinline__ int ann_of_poly(const PolyTables& t, int q) {
    int lo = 0, hi = t.NA;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.ann_poly[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// point d of the edge from vertex (xs,ys) to vertex (xe,ye): maskApi.c's upsampling loop in closed form
__device__ __forceinline__ void poly_edge_point(int xs, int ys, int xe, int ye, int d, int& u, int& v) {
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    if (dx >= dy) {
        const double s = dx > 0 ? (double)(ye - ys) / (double)dx : 0.0;
        const int t = flip ? dx - d : d;
        u = t + xs;
        v = (int)((double)ys + s * (double)t + .5);
    } else {
        const double s = (double)(xe - xs) / (double)dy;
        const int t = flip ? dy - d : d;
        v = t + ys;
        u = (int)((double)xs + s * (double)t + .5);
    }
}
// point j of the outline whose k edges start at eoff[0..k-1] (eoff[k] = the number of points)
__device__ __forceinline__ void poly_point(const int32_t* vxy, const int64_t* eoff, int k, int64_t j, int& u, int& v) {
    int lo = 0, hi = k;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (eoff[mid] <= j) lo = mid; else hi = mid;
    }
    const int e1 = lo + 1 == k ? 0 : lo + 1;
    poly_edge_point(vxy[2 * lo], vxy[2 * lo + 1], vxy[2 * e1], vxy[2 * e1 + 1], (int)(j - eoff[lo]), u, v);
}

__global__ __launch_bounds__(POLY_THREADS) void poly_generate_kernel(PolyTables t, PolyWork ws) {
    __shared__ long long wtot[4];
    __shared__ uint32_t ctot[2][4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const PolyRange pr = poly_range(t, q);
    const AnnRange ar = ann_range(t, ann_of_poly(t, q));
    const int k = pr.k;
    if (k == 0 || !ar.ok) {                                        // workgroup-uniform
        if (tid == 0) ws.cnt[q] = 0;
        return;
    }
    int32_t* vxy = ws.vxy + 2 * pr.v0;
    int64_t* eoff = ws.eoff + pr.v0 + q;
    const double* xy = t.xy + 2 * pr.v0;
    // ---- the vertices on the fine grid
    for (int i = tid; i < 2 * k; i += POLY_THREADS) vxy[i] = (int)(5.0 * xy[i] + .5);
    __syncthreads();
    // ---- the edges' first points: an exclusive prefix sum of max(dx,dy) + 1
    long long run = 0;
    for (int b = 0; b < k; b += POLY_THREADS) {
        const int e = b + tid;
        long long n = 0;
        if (e < k) {
            const int e1 = e + 1 == k ? 0 : e + 1;
            const int dx = abs(vxy[2 * e1] - vxy[2 * e]), dy = abs(vxy[2 * e1 + 1] - vxy[2 * e + 1]);
            n = (long long)max(dx, dy) + 1;
        }
        long long incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        const long long t0 = wtot[0], t1 = wtot[1], t2 = wtot[2], t3 = wtot[3];
        if (e < k) eoff[e] = run + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0) + incl - n;
        run += t0 + t1 + t2 + t3;
        __syncthreads();                                            // wtot is rewritten by the next round
    }
    if (tid == 0) eoff[k] = run;
    __syncthreads();
    // ---- one thread per point j >= 1: the pair (j-1, j)
    const int64_t total = run;
    const int H = (int)ar.H, W = (int)ar.W;
    uint32_t* out = ws.cross + pr.c0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t found = 0;
    int par = 0;
    for (int64_t b = 1; b < total; b += POLY_THREADS) {
        const int64_t j = b + tid;
        bool hit = false;
        uint32_t a = 0;
        if (j < total) {
            int u1, v1, u0, v0;
            poly_point(vxy, eoff, k, j, u1, v1);
            poly_point(vxy, eoff, k, j - 1, u0, v0);
            if (u1 != u0) {
                double xd = (double)(u1 < u0 ? u1 : u1 - 1);
                xd = (xd + .5) / 5.0 - .5;
                if (floor(xd) == xd && xd >= 0 && xd <= (double)(W - 1)) {
                    double yd = (double)(v1 < v0 ? v1 : v0);
                    yd = (yd + .5) / 5.0 - .5;
                    if (yd < 0) yd = 0; else if (yd > (double)H) yd = (double)H;
                    yd = ceil(yd);
                    a = (uint32_t)(int)xd * (uint32_t)H + (uint32_t)(int)yd;
                    hit = true;
                }
            }
        }
        const unsigned long long ball = __ballot(hit);
        if (lane == 0) ctot[par][w] = (uint32_t)__popcll(ball);
        __syncthreads();
        const uint32_t c0 = ctot[par][0], c1 = ctot[par][1], c2 = ctot[par][2], c3 = ctot[par][3];
        par ^= 1;                                                   // double-buffered: one barrier per round
        if (hit) {
            const uint32_t idx = found + (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0) + (uint32_t)__popcll(ball & lt);
            if (idx < (uint32_t)pr.cap && pr.c0 + idx < t.C) out[idx] = a;      // the polygon's slice and the list's capacity
        }
        found += c0 + c1 + c2 + c3;
    }
    if (tid == 0) ws.cnt[q] = (int32_t)min(found, (uint32_t)pr.cap);
}

// ---- sort: key[0..n) ascending; every thread of the workgroup calls it; ends with a barrier
template <typename KEYS>
__device__ __forceinline__ void poly_bitonic(KEYS key, uint32_t n) {
    for (uint32_t k = 2; (k >> 1) < n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t mask = j == (k >> 1) ? k - 1 : j;        // the first step of a merge mirrors, the others shift
            for (uint32_t i = threadIdx.x; i < n; i += POLY_THREADS) {
                const uint32_t l = i ^ mask;
                if (l > i && l < n) {
                    const uint32_t x = key[i], y = key[l];
                    if (y < x) { key[i] = y; key[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}
__device__ __forceinline__ void poly_sort(uint32_t* g, uint32_t n, uint32_t* lds) {
    if (n < 2) return;                                              // workgroup-uniform
    if (n <= (uint32_t)POLY_LDS_KEYS) {
        for (uint32_t i = threadIdx.x; i < n; i += POLY_THREADS) lds[i] = g[i];
        __syncthreads();
        poly_bitonic(lds, n);
        for (uint32_t i = threadIdx.x; i < n; i += POLY_THREADS) g[i] = lds[i];
        __syncthreads();
    } else {
        __syncthreads();                                            // the list was written by other threads of this workgroup
        poly_bitonic(g, n);
    }
}

__global__ __launch_bounds__(POLY_THREADS) void poly_sort_kernel(PolyTables t, PolyWork ws) {
    __shared__ uint32_t lds[POLY_LDS_KEYS];
    const int a = blockIdx.x, tid = threadIdx.x;
    const AnnRange ar = ann_range(t, a);
    uint32_t total = 0;
    for (int q = ar.q0; q < ar.q1; ++q) {
        const PolyRange pr = poly_range(t, q);
        const uint32_t n = (uint32_t)min(max(ws.cnt[q], 0), pr.cap);
        poly_sort(ws.cross + pr.c0, n, lds);
        total += n;
    }
    const uint32_t* cand = nullptr;
    if (ar.q1 - ar.q0 == 1) {
        cand = ws.cross + poly_range(t, ar.q0).c0;
    } else if (ar.q1 - ar.q0 > 1) {
        // the polygons' slices follow each other in the crossing list, so the annotation's candidate slice starts where its first
        // polygon's does and holds the sum of their capacities
        const int64_t base = poly_range(t, ar.q0).c0;
        uint32_t* dst = ws.cand + base;
        uint32_t at = 0;
        for (int q = ar.q0; q < ar.q1; ++q) {
            const PolyRange pr = poly_range(t, q);
            const uint32_t n = (uint32_t)min(max(ws.cnt[q], 0), pr.cap);
            for (uint32_t i = tid; i < n; i += POLY_THREADS)
                if (base + at + i < t.C) dst[at + i] = ws.cross[pr.c0 + i];
            at += n;
        }
        if (base + total > t.C) total = (uint32_t)max(t.C - base, (int64_t)0);
        __syncthreads();
        poly_sort(dst, total, lds);
        cand = dst;
    }
    if (tid == 0) {
        uint32_t lo = 0, hi = total;                                 // the first candidate >= H*W
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cand[mid] < ar.HW) lo = mid + 1; else hi = mid;
        }
        ws.ncand[a * 2 + 0] = (int32_t)total;
        ws.ncand[a * 2 + 1] = (int32_t)lo;
    }
}

// ---- the union's state at the candidates, streamed through the back end
struct PolyProducer {
    const uint32_t* cand;
    const uint32_t* cross;
    const int64_t* cross_off;
    const int32_t* cnt;
    int q0, q1;
    __device__ __forceinline__ int value(uint32_t p) const {
        const uint32_t c = cand[p];
        for (int q = q0; q < q1; ++q) {
            const uint32_t* lst = cross + cross_off[q];
            uint32_t lo = 0, hi = (uint32_t)cnt[q];                  // the number of crossings <= c
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lst[mid] <= c) lo = mid + 1; else hi = mid;
            }
            if (lo & 1u) return 1;
        }
        return 0;
    }
    __device__ __forceinline__ int before() const { return 0; }
    __device__ __forceinline__ uint32_t gpos(uint32_t p) const { return cand[p]; }
};
template <bool WRITE>
__global__ __launch_bounds__(POLY_THREADS) void poly_chars_kernel(PolyTables t, PolyWork ws, int64_t* __restrict__ sizes, const int64_t* __restrict__ offsets,
                                                                  uint8_t* __restrict__ chars, int64_t cap) {
    __shared__ RleShared sh;
    const int a = blockIdx.x;
    const AnnRange ar = ann_range(t, a);
    RleState st;
    const int64_t ob = WRITE ? offsets[a] : 0;
    if (ar.q1 > ar.q0) {
        const int64_t base = poly_range(t, ar.q0).c0;
        const uint32_t n = (uint32_t)max(ws.ncand[a * 2 + 1], 0);
        const PolyProducer prod{(ar.q1 - ar.q0 == 1 ? ws.cross : ws.cand) + base, ws.cross, t.cross_off, ws.cnt, ar.q0, ar.q1};
        if (base + n <= t.C) rle_stream<WRITE>(prod, n, sh, st, chars, ob, cap);
    }
    rle_finish<WRITE>(st, ar.HW, a, sizes, chars, ob, cap);
}

int64_t poly_align8(int64_t b) { return (b + 7) & ~(int64_t)7; }
struct PolyLayout { int64_t vxy, eoff, cnt, ncand, cross, cand, bytes; };
PolyLayout poly_layout(int64_t V, int NP, int NA, int64_t C) {
    PolyLayout l;
    int64_t at = 0;
    l.vxy = at; at += poly_align8(2 * V * 4);
    l.eoff = at; at += (V + NP) * 8;
    l.cnt = at; at += poly_align8((int64_t)NP * 4);
    l.ncand = at; at += (int64_t)NA * 8;
    l.cross = at; at += poly_align8(C * 4);
    l.cand = at; at += poly_align8(C * 4);
    l.bytes = at;
    return l;
}

}  // namespace

extern "C" int64_t umr_poly_rle_workspace(int64_t n_vertices, int n_polygons, int n_annotations, int64_t crossing_capacity) {
    if (n_vertices < 0 || n_polygons < 0 || n_annotations < 0 || crossing_capacity < 0) return -1;
    return poly_layout(n_vertices, n_polygons, n_annotations, crossing_capacity).bytes;
}

extern "C" int umr_poly_rle(const double* xy, const int64_t* poly_offsets, const int64_t* ann_polys, const int64_t* ann_sizes,
                            const int64_t* cross_offsets, int64_t n_vertices, int n_polygons, int n_annotations, int64_t crossing_capacity,
                            int phases, int64_t* sizes, const int64_t* offsets, uint8_t* chars, int64_t chars_capacity, void* workspace,
                            int64_t workspace_bytes, umr_stream_t stream) {
    UMR_CHECK_ARG(xy && poly_offsets && ann_polys && ann_sizes && cross_offsets && workspace, "poly_rle: bad arguments (a null table or workspace)");
    UMR_CHECK_ARG(n_vertices >= 0 && n_polygons >= 0 && n_annotations > 0 && crossing_capacity >= 0, "poly_rle: bad arguments (extents)");
    UMR_CHECK_ARG(phases > 0 && phases < 8, "poly_rle: phases is a mask of 1 (generate), 2 (sort), 4 (characters)");
    UMR_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "poly_rle: the workspace must be 8-byte aligned");
    const PolyLayout l = poly_layout(n_vertices, n_polygons, n_annotations, crossing_capacity);
    UMR_CHECK_ARG(workspace_bytes >= l.bytes, "poly_rle: the workspace is smaller than umr_poly_rle_workspace reports");
    if (phases & 4)
        UMR_CHECK_ARG(rle_buffers_ok(sizes, offsets, chars, chars_capacity),
                      "poly_rle: the measure pass needs sizes; the write pass needs offsets, chars and a positive chars_capacity");
    char* base = (char*)workspace;
    const PolyTables t{xy, poly_offsets, ann_polys, ann_sizes, cross_offsets, n_vertices, crossing_capacity, n_polygons, n_annotations};
    const PolyWork ws{(int32_t*)(base + l.vxy), (int64_t*)(base + l.eoff), (int32_t*)(base + l.cnt), (int32_t*)(base + l.ncand),
                      (uint32_t*)(base + l.cross), (uint32_t*)(base + l.cand)};
    hipStream_t s = (hipStream_t)stream;
    if ((phases & 1) && n_polygons > 0) {
        hipLaunchKernelGGL(poly_generate_kernel, dim3(n_polygons), dim3(POLY_THREADS), 0, s, t, ws);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 2) {
        hipLaunchKernelGGL(poly_sort_kernel, dim3(n_annotations), dim3(POLY_THREADS), 0, s, t, ws);
        UMR_LAUNCH_CHECK();
    }
    if (phases & 4) {
        if (chars) hipLaunchKernelGGL(poly_chars_kernel<true>, dim3(n_annotations), dim3(POLY_THREADS), 0, s, t, ws, sizes, offsets, chars, chars_capacity);
        else hipLaunchKernelGGL(poly_chars_kernel<false>, dim3(n_annotations), dim3(POLY_THREADS), 0, s, t, ws, sizes, offsets, chars, chars_capacity);
        UMR_LAUNCH_CHECK();
    }
    return UMR_OK;
}
