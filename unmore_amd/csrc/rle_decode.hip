// COCO run-length strings (pycocotools' maskApi.c format, see rle.hip) back to masks on the device, and the largest 4-connected
// component of a decoded mask -- what utils/preprocess_votecut.py:71-94 (top-1 annotation, cv2.connectedComponentsWithStats(mask, 4),
// np.argmax of the areas) and utils/vis_votecut.py:57-79 (union of an image's annotations) compute on the host.
//
// rle_parse_kernel, one workgroup per string: a character without 0x20 ends a number; the ends are flagged and ranked in string order
// (shuffle scan inside a wave, four wave totals through LDS); the thread at an end assembles its number from the at most 7 characters
// before it; counts[i] = x[i] + counts[i-2] for i > 2 is one prefix sum over the odd positions and one over the even positions from 2
// on; the run starts are a third prefix sum.  A character outside the format, a number of more than 7 characters, a count outside
// [0, H*W] and counts that do not sum to H*W give a non-zero status; such a record is never painted or labelled.
// rle_union_paint_kernel (mode 0): per pixel of the row-major output, j = x*H + y is looked up in the run starts of every record of
// the group (the LAST run that starts at or before j: zero-length runs repeat a start); odd run = set.
// rle_largest_kernel (mode 1), one workgroup per mask: the runs of ones are split at column boundaries into segments (j0, j1), in
// column-major order; two segments are united when they sit in neighbouring columns and their rows overlap, or touch inside a column
// (a zero-length run of zeros); union-find with integer atomicMin, parents in LDS when the segments fit, else in the workgroup's own
// workspace slice; the root of a component is its smallest segment index, whatever the order of the unions.  Per root: area (integer
// sum of segment lengths) and first pixel in raster order (minimum of y0*W + x); kept = largest area, ties to the earliest first
// pixel.  No flag or wait between workgroups, no float atomics; every loop is bounded by the segment count; every store is guarded by
// the record's own output, number and segment slice.  The same input gives the same bytes on every run.
#include "umr_common.h"
#include <limits.h>

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_LDS_SEGS = 12288;                 // parents in LDS up to this many segments (48 KiB)
constexpr int RD_SEG_FIELDS = 5;                   // j0, j1, area, first, parent: int32 each
enum { RD_BAD_CHAR = 1, RD_BAD_COUNT = 2, RD_BAD_SUM = 4, RD_BAD_TABLE = 8 };

struct RdScan {
    long long wtot[2][4];                          // double-buffered by call parity: one barrier per scan
};

// inclusive scan of v over the workgroup in thread order; `total` = the sum of all 256 values.  Called by every thread.
__device__ __forceinline__ long long rd_scan(long long v, RdScan& sc, int& par, long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) sc.wtot[par][w] = incl;
    __syncthreads();
    const long long s0 = sc.wtot[par][0], s1 = sc.wtot[par][1], s2 = sc.wtot[par][2], s3 = sc.wtot[par][3];
    par ^= 1;
    total = s0 + s1 + s2 + s3;
    return incl + (w > 0 ? s0 : 0) + (w > 1 ? s1 : 0) + (w > 2 ? s2 : 0);
}

struct RdOut {                                     // one output mask, checked against the packed buffer
    int H, W;
    uint32_t HW;
    int64_t off;
    bool ok;
};
__device__ __forceinline__ RdOut rd_out(const int64_t* __restrict__ out_desc, int g, int64_t out_bytes) {
    const int64_t H = out_desc[g * 3 + 0], W = out_desc[g * 3 + 1], off = out_desc[g * 3 + 2];
    RdOut o;
    o.ok = H > 0 && W > 0 && H < ((int64_t)1 << 31) && W < ((int64_t)1 << 31) && H * W < ((int64_t)1 << 31) && off >= 0 && off <= out_bytes &&
           H * W <= out_bytes - off;
    o.H = o.ok ? (int)H : 1;
    o.W = o.ok ? (int)W : 1;
    o.HW = o.ok ? (uint32_t)(H * W) : 0u;
    o.off = off;
    return o;
}

// the number of starts <= j, minus one: the last run that starts at or before j (starts[0] == 0)
__device__ __forceinline__ int rd_find_run(const uint32_t* __restrict__ starts, int n, uint32_t j) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (starts[m] <= j) lo = m + 1; else hi = m;
    }
    return lo - 1;
}

__global__ __launch_bounds__(RD_THREADS) void rle_parse_kernel(const uint8_t* __restrict__ chars, const int64_t* __restrict__ char_offsets,
                                                               int64_t total_chars, const int64_t* __restrict__ out_desc,
                                                               const int32_t* __restrict__ group_start, int G, int64_t out_bytes,
                                                               int32_t* __restrict__ status, int32_t* __restrict__ nruns, long long* __restrict__ num,
                                                               uint32_t* __restrict__ starts) {
    __shared__ RdScan sc;
    __shared__ int bad_s;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) bad_s = 0;
    // the record's group: the last g with group_start[g] <= k
    int ga = 0, gb = G + 1;
    while (ga < gb) {
        const int m = (ga + gb) >> 1;
        if (group_start[m] <= k) ga = m + 1; else gb = m;
    }
    const int g = ga - 1;
    const int64_t c0 = char_offsets[k], c1 = char_offsets[k + 1];
    bool table_ok = g >= 0 && g < G && c0 >= 0 && c0 <= c1 && c1 <= total_chars && c1 - c0 < ((int64_t)1 << 31);
    RdOut o;
    o.ok = false;
    if (table_ok) o = rd_out(out_desc, g, out_bytes);
    if (!table_ok || !o.ok) {                      // workgroup-uniform
        if (tid == 0) { status[k] = RD_BAD_TABLE; nruns[k] = 0; }
        return;
    }
    __syncthreads();
    const uint8_t* s = chars + c0;
    const int n = (int)(c1 - c0);
    const int64_t nb = c0 + k;                      // this record's slice of num / starts: n + 1 slots
    const long long HW = o.HW;
    int par = 0, bad = 0;
    long long nn = 0;                               // numbers so far
    // ---- ends -> numbers
    for (int base = 0; base < n; base += RD_THREADS) {
        const int p = base + tid;
        const bool valid = p < n;
        const int c = valid ? (int)s[p] - 48 : 0x20;
        const bool okc = c >= 0 && c < 64;
        if (!okc) bad |= RD_BAD_CHAR;
        const bool end = valid && okc && !(c & 0x20);
        if (valid && p == n - 1 && !end) bad |= RD_BAD_CHAR;        // the string stops inside a number
        long long x = 0;
        if (end) {
            int len = 1;
            while (len < 8 && p - len >= 0) {
                const int d = (int)s[p - len] - 48;
                if (d < 0 || d > 63 || !(d & 0x20)) break;
                ++len;
            }
            if (len == 8) {
                bad |= RD_BAD_COUNT;                                // more than 7 groups: beyond 32 bits
            } else {
                for (int i = 0; i < len; ++i) x |= (long long)(((int)s[p - len + 1 + i] - 48) & 0x1f) << (5 * i);
                if (c & 0x10) x |= -1ll << (5 * len);
                if (x < -((long long)1 << 31) || x > ((long long)1 << 31)) { bad |= RD_BAD_COUNT; x = 0; }
            }
        }
        long long tot;
        const long long incl = rd_scan(end ? 1 : 0, sc, par, tot);
        if (end) num[nb + nn + incl - 1] = x;                       // at most one number per character
        nn += tot;
    }
    __syncthreads();
    // ---- numbers -> counts -> run starts
    long long ce = 0, co = 0, st = 0;
    for (long long base = 0; base < nn; base += RD_THREADS) {
        const long long i = base + tid;
        const bool valid = i < nn;
        const long long x = valid ? num[nb + i] : 0;
        long long te, to, ts;
        const long long ie = rd_scan(valid && i >= 2 && !(i & 1) ? x : 0, sc, par, te);
        const long long io = rd_scan(valid && (i & 1) ? x : 0, sc, par, to);
        long long cnt = !valid ? 0 : i == 0 ? x : (i & 1) ? co + io : ce + ie;
        ce += te; co += to;
        if (cnt < 0 || cnt > HW) { bad |= RD_BAD_COUNT; cnt = 0; }
        const long long is = rd_scan(cnt, sc, par, ts);
        if (valid) starts[nb + i] = (uint32_t)(st + is - cnt);
        st += ts;
    }
    if (st != HW) bad |= RD_BAD_SUM;
    if (bad) atomicOr(&bad_s, bad);
    __syncthreads();
    if (tid == 0) { status[k] = bad_s; nruns[k] = (int)nn; }
}

__global__ __launch_bounds__(RD_THREADS) void rle_union_paint_kernel(const int64_t* __restrict__ char_offsets, const int64_t* __restrict__ out_desc,
                                                                     const int32_t* __restrict__ group_start, int K, const int32_t* __restrict__ status,
                                                                     const int32_t* __restrict__ nruns, const uint32_t* __restrict__ starts,
                                                                     uint8_t* __restrict__ out, int64_t out_bytes, int value) {
    const int g = blockIdx.x;
    const RdOut o = rd_out(out_desc, g, out_bytes);
    if (!o.ok) return;
    const int r0 = max(group_start[g], 0), r1 = min(group_start[g + 1], K);
    uint8_t* dst = out + o.off;
    const bool dwords = (((uintptr_t)dst) & 3) == 0;
    for (uint32_t p0 = (blockIdx.y * RD_THREADS + threadIdx.x) * 4u; p0 < o.HW; p0 += gridDim.y * RD_THREADS * 4u) {
        uint32_t word = 0;
        const uint32_t np = min(4u, o.HW - p0);
        for (uint32_t e = 0; e < np; ++e) {
            const uint32_t p = p0 + e, y = p / (uint32_t)o.W, x = p - y * (uint32_t)o.W, j = x * (uint32_t)o.H + y;
            int v = 0;
            for (int r = r0; r < r1 && !v; ++r) {
                if (status[r] != 0) continue;
                v = rd_find_run(starts + char_offsets[r] + r, nruns[r], j) & 1;
            }
            if (v) word |= (uint32_t)(value & 0xff) << (8 * e);
        }
        if (dwords && np == 4) {
            *(uint32_t*)(dst + p0) = word;
        } else {
            for (uint32_t e = 0; e < np; ++e) dst[p0 + e] = (uint8_t)(word >> (8 * e));
        }
    }
}

__device__ __forceinline__ int rd_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// parents only ever decrease, so a chain has at most `a` links
__device__ __forceinline__ int rd_root(const int* par, int a) {
    int p = rd_ld(par + a);
    while (p != a) { a = p; p = rd_ld(par + a); }
    return a;
}
// Lock-free union (Playne & Equalizer): hang the larger root under the smaller with atomicMin; a lost race continues from the value
// that won.  a + b decreases with every retry.
__device__ __forceinline__ void rd_union(int* par, int a, int b) {
    bool done;
    do {
        a = rd_root(par, a);
        b = rd_root(par, b);
        if (a < b) {
            const int old = atomicMin(par + b, a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(par + a, b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

__global__ __launch_bounds__(RD_THREADS) void rle_largest_kernel(const int64_t* __restrict__ char_offsets, const int64_t* __restrict__ out_desc,
                                                                 const int32_t* __restrict__ group_start, const int64_t* __restrict__ seg_offsets,
                                                                 int64_t total_segments, int K, int32_t* __restrict__ status,
                                                                 const int32_t* __restrict__ nruns, const uint32_t* __restrict__ starts,
                                                                 int* __restrict__ seg_ws, uint8_t* __restrict__ out, int64_t out_bytes, int value,
                                                                 int32_t* __restrict__ info) {
    __shared__ int par_lds[RD_LDS_SEGS];
    __shared__ RdScan sc;
    __shared__ unsigned long long best_w[4];
    __shared__ int cnt_w[4];
    __shared__ int best_root_s;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) { info[g * 2] = 0; info[g * 2 + 1] = 0; best_root_s = -1; }
    const RdOut o = rd_out(out_desc, g, out_bytes);
    if (!o.ok) return;
    uint8_t* dst = out + o.off;
    {   // all zero first: head bytes up to a dword boundary, dwords, tail bytes
        const uint32_t head = min((uint32_t)((4 - ((uintptr_t)dst & 3)) & 3), o.HW), nd = (o.HW - head) >> 2, tail0 = head + nd * 4;
        if (tid < (int)head) dst[tid] = 0;
        for (uint32_t i = tid; i < nd; i += RD_THREADS) *(uint32_t*)(dst + head + (size_t)i * 4) = 0u;
        if (tail0 + tid < o.HW && tid < 4) dst[tail0 + tid] = 0;
    }
    const int r = group_start[g];
    const int64_t so = seg_offsets[g], se = seg_offsets[g + 1];
    const int r_end = group_start[g + 1];
    if (r_end - r != 1 || r < 0 || r >= K || so < 0 || se < so || se > total_segments || se - so >= ((int64_t)1 << 31)) {
        // not exactly one record, or a segment slice out of range: the group's records say so (the host cannot see the table)
        for (int q = max(r, 0) + tid; q < min(r_end, K); q += RD_THREADS) status[q] = RD_BAD_TABLE;
        return;
    }
    if (status[r] != 0) return;                                     // workgroup-uniform: written by the parse launch
    const int cap = (int)(se - so);
    const int n = nruns[r];
    const uint32_t* s = starts + char_offsets[r] + r;
    int* j0 = seg_ws + so * RD_SEG_FIELDS;
    int* j1 = j0 + cap;
    int* area = j1 + cap;
    int* first = area + cap;
    int* gpar = first + cap;
    const uint32_t H = (uint32_t)o.H, W = (uint32_t)o.W;
    // ---- runs of ones -> segments, in column-major order
    int par = 0;
    const int m = n >> 1;
    long long S = 0;
    for (int base = 0; base < m; base += RD_THREADS) {
        const int t = base + tid;
        uint32_t a = 0, b = 0, xs = 0;
        long long cnt = 0;
        if (t < m) {
            const int i = 2 * t + 1;
            a = s[i];
            b = i + 1 < n ? s[i + 1] : o.HW;
            if (b > a) { xs = a / H; cnt = (long long)((b - 1) / H - xs) + 1; }
        }
        long long tot;
        const long long first_idx = S + rd_scan(cnt, sc, par, tot) - cnt;
        for (long long c = 0; c < cnt; ++c) {
            const long long idx = first_idx + c;
            if (idx >= cap) break;
            const uint32_t x = xs + (uint32_t)c;
            j0[idx] = (int)max(a, x * H);
            j1[idx] = (int)(min(b, (x + 1) * H) - 1);
            area[idx] = 0;
            first[idx] = INT_MAX;
        }
        S += tot;
    }
    if (S > cap) {                                                  // cannot happen with the caller's bound nchars/2 + 1 + W
        if (tid == 0) status[r] = RD_BAD_TABLE;
        return;
    }
    const int ns = (int)S;
    if (ns == 0) return;                                            // an empty mask: (0, 0), all zero
    int* pr = ns <= RD_LDS_SEGS ? par_lds : gpar;
    for (int i = tid; i < ns; i += RD_THREADS) pr[i] = i;
    __syncthreads();
    // ---- unions
    for (int i = tid; i < ns; i += RD_THREADS) {
        const uint32_t a = (uint32_t)j0[i], b = (uint32_t)j1[i], x = a / H;
        if (i > 0 && (uint32_t)j1[i - 1] + 1 == a && a != x * H) rd_union(pr, i, i - 1);
        if (x > 0) {
            const int lo = (int)(a - H), hi = (int)(b - H);
            int l = 0, h = i;
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (j1[mid] < lo) l = mid + 1; else h = mid;
            }
            for (int t = l; t < i && j0[t] <= hi; ++t) rd_union(pr, i, t);
        }
    }
    __syncthreads();
    for (int i = tid; i < ns; i += RD_THREADS) {
        const int root = rd_root(pr, i);
        __hip_atomic_store(pr + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // still an ancestor for a concurrent walk
    }
    __syncthreads();
    // ---- area and first raster pixel per root
    for (int i = tid; i < ns; i += RD_THREADS) {
        const uint32_t a = (uint32_t)j0[i], b = (uint32_t)j1[i], x = a / H, y0 = a - x * H;
        const int root = rd_ld(pr + i);
        atomicAdd(area + root, (int)(b - a + 1));
        atomicMin(first + root, (int)(y0 * W + x));
    }
    __syncthreads();
    // ---- the number of roots; the root of largest area, ties to the earliest first pixel (first pixels are distinct)
    unsigned long long best = 0;
    int cnt = 0;
    for (int i = tid; i < ns; i += RD_THREADS) {
        if (rd_ld(pr + i) != i) continue;
        ++cnt;
        const unsigned long long key = ((unsigned long long)(uint32_t)rd_ld(area + i) << 32) | (0xffffffffu - (uint32_t)rd_ld(first + i));
        best = key > best ? key : best;
    }
#pragma unroll
    for (int q = 32; q > 0; q >>= 1) {
        const unsigned long long ob = __shfl_xor(best, q, 64);
        best = ob > best ? ob : best;
        cnt += __shfl_xor(cnt, q, 64);
    }
    if (lane == 0) { best_w[w] = best; cnt_w[w] = cnt; }
    __syncthreads();
    best = max(max(best_w[0], best_w[1]), max(best_w[2], best_w[3]));
    cnt = cnt_w[0] + cnt_w[1] + cnt_w[2] + cnt_w[3];
    for (int i = tid; i < ns; i += RD_THREADS) {
        if (rd_ld(pr + i) != i) continue;
        const unsigned long long key = ((unsigned long long)(uint32_t)rd_ld(area + i) << 32) | (0xffffffffu - (uint32_t)rd_ld(first + i));
        if (key == best) best_root_s = i;
    }
    __syncthreads();
    const int keep = best_root_s;
    if (tid == 0) { info[g * 2] = cnt; info[g * 2 + 1] = (int)(best >> 32); }
    if (keep < 0) return;
    // ---- paint the kept component: one wave per segment, lanes down its rows
    for (int i = w; i < ns; i += RD_THREADS / 64) {
        if (rd_ld(pr + i) != keep) continue;
        const uint32_t a = (uint32_t)j0[i], b = (uint32_t)j1[i], x = a / H, y0 = a - x * H, y1 = b - x * H;
        for (uint32_t y = y0 + lane; y <= y1; y += 64) dst[(size_t)y * W + x] = (uint8_t)value;
    }
}

int64_t rd_align8(int64_t v) { return (v + 7) & ~(int64_t)7; }
bool rd_sizes_ok(int K, int64_t total_chars, int64_t total_segments) {
    return K >= 0 && total_chars >= 0 && total_segments >= 0 && total_chars < ((int64_t)1 << 40) && total_segments < ((int64_t)1 << 40);
}

}  // namespace

int umr_rle_parse_launch(const uint8_t* chars, const int64_t* char_offsets, int K, int64_t total_chars, const int64_t* out_desc,
                         const int32_t* group_start, int G, int64_t out_bytes, int32_t* status, int32_t* nruns, long long* num,
                         uint32_t* starts, hipStream_t stream) {
    if (K <= 0) return UMR_OK;
    hipLaunchKernelGGL(rle_parse_kernel, dim3(K), dim3(RD_THREADS), 0, stream, chars, char_offsets, total_chars, out_desc, group_start, G,
                       out_bytes, status, nruns, num, starts);
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}

extern "C" int64_t umr_rle_decode_workspace(int K, int64_t total_chars, int64_t total_segments, int mode) {
    if (!rd_sizes_ok(K, total_chars, total_segments) || (mode != 0 && mode != 1)) return -1;
    const int64_t slots = total_chars + K;
    return rd_align8((int64_t)K * 4) + slots * 8 + rd_align8(slots * 4) + (mode == 1 ? rd_align8(total_segments * RD_SEG_FIELDS * 4) : 0) + 8;
}

extern "C" int umr_rle_decode(const uint8_t* chars, const int64_t* char_offsets, int K, int64_t total_chars, const int64_t* out_desc,
                              const int32_t* group_start, const int64_t* seg_offsets, int G, int64_t max_pixels, int64_t total_segments,
                              uint8_t* out, int64_t out_bytes, int value, int mode, int32_t* status, int32_t* info, void* workspace,
                              int64_t workspace_bytes, umr_stream_t stream) {
    UMR_CHECK_ARG(G > 0 && rd_sizes_ok(K, total_chars, total_segments), "rle_decode: bad sizes");
    UMR_CHECK_ARG(mode == 0 || mode == 1, "rle_decode: mode is 0 (union of a group) or 1 (largest 4-connected component)");
    UMR_CHECK_ARG(value >= 0 && value <= 255, "rle_decode: value is a byte");
    UMR_CHECK_ARG(max_pixels > 0 && max_pixels < ((int64_t)1 << 31), "rle_decode: H * W must be positive and below 2^31");
    UMR_CHECK_ARG(out_desc && group_start && out && out_bytes > 0 && workspace, "rle_decode: null table, output or workspace");
    UMR_CHECK_ARG(K == 0 || (chars && char_offsets && status), "rle_decode: null strings, offsets or status");
    UMR_CHECK_ARG(mode == 0 || (K == G && seg_offsets && info), "rle_decode: mode 1 takes one record per group, segment offsets and info");
    UMR_CHECK_ARG(workspace_bytes >= umr_rle_decode_workspace(K, total_chars, total_segments, mode), "rle_decode: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int64_t slots = total_chars + K;
    char* ws = (char*)workspace;
    int32_t* nruns = (int32_t*)ws;
    long long* num = (long long*)(ws + rd_align8((int64_t)K * 4));
    uint32_t* starts = (uint32_t*)((char*)num + slots * 8);
    int* seg_ws = (int*)((char*)starts + rd_align8(slots * 4));
    if (K > 0) {
        hipLaunchKernelGGL(rle_parse_kernel, dim3(K), dim3(RD_THREADS), 0, s, chars, char_offsets, total_chars, out_desc, group_start, G, out_bytes,
                           status, nruns, num, starts);
        UMR_LAUNCH_CHECK();
    }
    if (mode == 0) {
        const int64_t tiles = (max_pixels + RD_THREADS * 4 - 1) / (RD_THREADS * 4);
        hipLaunchKernelGGL(rle_union_paint_kernel, dim3(G, (unsigned)(tiles < 1024 ? tiles : 1024)), dim3(RD_THREADS), 0, s, char_offsets, out_desc,
                           group_start, K, status, nruns, starts, out, out_bytes, value);
    } else {
        hipLaunchKernelGGL(rle_largest_kernel, dim3(G), dim3(RD_THREADS), 0, s, char_offsets, out_desc, group_start, seg_offsets, total_segments, K,
                           status, nruns, starts, seg_ws, out, out_bytes, value, info);
    }
    UMR_LAUNCH_CHECK();
    return UMR_OK;
}
