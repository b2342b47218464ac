"""COCO run-length encoding of binary masks: the `segmentation` of the records object scoring writes (object_scoring.py:166-170,257-272).

The format is pycocotools' (maskApi.c).  For a mask [H,W] of 0/1 the pixels are taken in column-major order, j = x*H + y; `counts` are the
lengths of the alternating runs, starting with a run of zeros (0 when pixel 0 is set; an all-zero mask is the single count H*W).  The
string writes, for run i, x = counts[i] - (counts[i-2] if i > 2 else 0) as a signed number in 5-bit groups, low group first: after
c = x & 0x1f and x >>= 5 (arithmetic) another group follows iff (x != -1 if c & 0x10 else x != 0); a group that is followed by another
has 0x20 set; every group is the character chr(c + 48).  A record is {"size": [H, W], "counts": str}.

`encode` / `encode_pasted` run on the device (csrc/rle.hip): a measure pass, one small read of the sizes, a write pass into a packed
buffer, one read of the characters -- nothing image-sized crosses to the host.  `from_polygons` (csrc/poly_rle.hip) makes the records
of polygon segmentations by pycocotools' annToRLE rule through the same two passes.  The *_numpy functions restate the format and the
polygon rule on the CPU: what the tests compare the kernels against and what a host without a GPU reads the file back with."""
import ctypes

import numpy as np


# ---------------------------------------------------------------------------------------------------------------- the format on the CPU
def mask_to_counts(mask):
    """[H,W] 0/1 -> the run lengths (int64 array), column-major, starting with zeros"""
    m = np.asarray(mask)
    assert m.ndim == 2, "a mask is [H, W]"
    flat = (m != 0).reshape(-1, order="F") if m.size else np.zeros(0, bool)
    change = np.flatnonzero(np.diff(np.concatenate([[False], flat]).astype(np.int8)) != 0)   # position j: pixel j differs from pixel j-1
    bounds = np.concatenate([[0], change, [flat.size]]).astype(np.int64)
    return np.diff(bounds)


def counts_to_string(counts):
    out = bytearray()
    cs = [int(c) for c in counts]
    for i, c in enumerate(cs):
        x = c - (cs[i - 2] if i > 2 else 0)
        more = True
        while more:
            g = x & 0x1f
            x >>= 5
            more = (x != -1) if (g & 0x10) else (x != 0)
            if more:
                g |= 0x20
            out.append(g + 48)
    return out.decode("ascii")


def string_to_counts(s):
    if isinstance(s, str):
        s = s.encode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            g = s[p] - 48
            x |= (g & 0x1f) << (5 * k)
            more = bool(g & 0x20)
            p += 1
            k += 1
            if not more and (g & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return np.asarray(counts, dtype=np.int64)


def encode_numpy(mask):
    m = np.asarray(mask)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": counts_to_string(mask_to_counts(m))}


def decode_numpy(rle):
    """record -> [H,W] u8"""
    H, W = rle["size"]
    counts = string_to_counts(rle["counts"])
    assert int(counts.sum()) == H * W and (counts >= 0).all(), "counts do not cover the mask"
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)
    return flat.reshape((H, W), order="F")


def area(rle):
    """number of set pixels (pycocotools' `area`)"""
    return int(string_to_counts(rle["counts"])[1::2].sum())


def to_bbox(rle):
    """pycocotools' `toBbox`: [x, y, w, h] of the set pixels as floats, all zero for an empty mask"""
    H, W = rle["size"]
    counts = string_to_counts(rle["counts"])
    ends = np.cumsum(counts)
    s, e = (ends - counts)[1::2], ends[1::2] - 1          # first and last pixel of every run of ones
    keep = e >= s
    s, e = s[keep], e[keep]
    if len(s) == 0:
        return [0.0, 0.0, 0.0, 0.0]
    xs, xe = s // H, e // H
    x1, x2 = int(xs.min()), int(xe.max())
    if (xe > xs).any():                                     # a run that crosses a column boundary touches the last and the first row
        y1, y2 = 0, H - 1
    else:
        y1, y2 = int((s % H).min()), int((e % H).max())
    return [float(x1), float(y1), float(x2 - x1 + 1), float(y2 - y1 + 1)]


# ---------------------------------------------------------------------------------------------------------------- polygons on the CPU
# pycocotools' annToRLE for a polygon segmentation: maskApi.c's rleFrPoly per polygon, then rleMerge (union) over the annotation's
# polygons, restated sequentially, loop by loop, in plain Python floats (IEEE doubles; int() truncates toward zero as C's (int) does).
# A polygon's vertices are scaled by 5, every edge is walked point by point on that fine grid, a "crossing" is recorded wherever the
# walk steps over the centre line of a pixel column inside the image, at the pixel row the walk is at; pixel p = x*H + y (column-major)
# is set iff an odd number of crossings lie at or before it.
POLY_SCALE = 5.0
POLY_MAX_COORD = float(1 << 20)


def _poly_vertices(xy):
    """step 1: flat [x0, y0, x1, y1, ...] -> integer vertices on the fine grid (lists x, y of k ints, not yet closed)"""
    k = len(xy) // 2
    x = [int(POLY_SCALE * float(xy[2 * j]) + .5) for j in range(k)]
    y = [int(POLY_SCALE * float(xy[2 * j + 1]) + .5) for j in range(k)]
    return x, y


def polygon_points_numpy(xy):
    """steps 1-2: the points (u, v) along the closed outline, all edges concatenated in order (two int lists)"""
    x, y = _poly_vertices(xy)
    k = len(x)
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = float(ye - ys) / dx if dx > 0 else 0.0        # a zero-length edge: one point, its v is never used
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    return u, v


def polygon_crossings_numpy(xy, h, w):
    """steps 1-3: the crossings a = xd*h + yd of one polygon on an h x w image, in the order the outline meets them (int64 array;
    a value can equal h*w)"""
    u, v = polygon_points_numpy(xy)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / POLY_SCALE - .5
        if np.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / POLY_SCALE - .5
        if yd < 0:
            yd = 0.0
        elif yd > h:
            yd = float(h)
        yd = np.ceil(yd)
        out.append(int(xd) * h + int(yd))
    return np.asarray(out, dtype=np.int64)


def polygon_mask_numpy(xy, h, w):
    """step 4: [h, w] u8, pixel p = x*h + y set iff the number of crossings <= p is odd"""
    a = polygon_crossings_numpy(xy, h, w)
    hits = np.bincount(a[a < h * w], minlength=h * w)
    return (np.cumsum(hits) & 1).astype(np.uint8).reshape((h, w), order="F")


def _check_polygons(segmentations, sizes, what):
    """the restrictions, before anything is computed: (list of lists of float64 arrays, list of (H, W))"""
    n = len(segmentations)
    if len(sizes) == 2 and not isinstance(sizes[0], (list, tuple, np.ndarray)):
        sizes = [sizes] * n
    if len(sizes) != n:
        raise ValueError(f"{what}: {n} segmentations, {len(sizes)} sizes")
    polys, out_sizes = [], []
    for i, (seg, size) in enumerate(zip(segmentations, sizes)):
        if isinstance(seg, dict) or not isinstance(seg, (list, tuple)) or any(not isinstance(p, (list, tuple, np.ndarray)) for p in seg):
            raise ValueError(f"{what}: segmentation {i} is not a polygon segmentation (a list of flat coordinate lists)")
        H, W = int(size[0]), int(size[1])
        if H <= 0 or W <= 0 or H * W >= 1 << 31:
            raise ValueError(f"{what}: segmentation {i}: size {[H, W]} must be positive with H*W < 2^31")
        mine = []
        for q, p in enumerate(seg):
            c = np.asarray(p, dtype=np.float64).reshape(-1)
            if c.size == 0 or c.size % 2:
                raise ValueError(f"{what}: segmentation {i}, polygon {q}: {c.size} coordinates; a non-empty list of x, y pairs is expected")
            if not np.isfinite(c).all():
                raise ValueError(f"{what}: segmentation {i}, polygon {q}: a coordinate is not finite")
            if (np.abs(c) > POLY_MAX_COORD).any():
                raise ValueError(f"{what}: segmentation {i}, polygon {q}: a coordinate is beyond 2^20 in magnitude")
            mine.append(c)
        polys.append(mine)
        out_sizes.append((H, W))
    return polys, out_sizes


def from_polygons_numpy(segmentations, sizes):
    """step 5: the records of polygon segmentations on the CPU.  segmentations[i]: a list of flat [x0, y0, x1, y1, ...] lists; sizes:
    one (H, W) or one per segmentation.  The mask is the OR of the polygons' masks, the record its canonical string."""
    polys, sizes = _check_polygons(segmentations, sizes, "from_polygons_numpy")
    out = []
    for mine, (H, W) in zip(polys, sizes):
        m = np.zeros((H, W), np.uint8)
        for c in mine:
            m |= polygon_mask_numpy(c, H, W)
        out.append(encode_numpy(m))
    return out


# ---------------------------------------------------------------------------------------------------------------- on the device
def _two_pass(launch, K, H, W, device):
    """measure -> sizes to the host -> packed write -> characters to the host; `launch(sizes, offsets, chars, capacity)` enqueues a pass"""
    import torch
    sizes = torch.empty((K, 2), dtype=torch.int64, device=device)
    launch(sizes, None, None, 0)
    nchars = sizes[:, 1].cpu().numpy()                                       # device-to-host read 1: K pairs
    offsets = np.concatenate([[0], np.cumsum(nchars)]).astype(np.int64)
    total = int(offsets[-1])
    chars = torch.empty((total,), dtype=torch.uint8, device=device)
    launch(None, torch.from_numpy(offsets[:-1].copy()).to(device), chars, total)
    text = chars.cpu().numpy().tobytes().decode("ascii")                     # device-to-host read 2: the packed strings
    return [{"size": [int(H), int(W)], "counts": text[offsets[k]:offsets[k + 1]]} for k in range(K)]


def encode(masks):
    """device u8 / bool masks [K,H,W] or [H,W] (0 = clear) -> list of K records (one record for [H,W])"""
    import torch
    from . import _lib as L
    from .ops import _need_gpu, _p, _stream
    _need_gpu(masks)
    single = masks.dim() == 2
    m = masks[None] if single else masks
    assert m.dim() == 3 and m.dtype in (torch.uint8, torch.bool), "masks: [K,H,W] or [H,W], u8 or bool"
    m = m.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    K, H, W = m.shape
    if K == 0:
        return []

    def launch(sizes, offsets, chars, cap):
        L.check(L.lib().umr_rle_encode(_p(m), K, H, W, _p(sizes), _p(offsets), _p(chars), cap, _stream()), "umr_rle_encode")
    out = _two_pass(launch, K, H, W, m.device)
    return out[0] if single else out


def encode_pasted(sdf, center, int_boxes, select, H, W):
    """the records of the pasted union masks `umr_mask_paste` would write for the proposals `select` (int64 indices into the N proposals),
    without writing the masks: sdf [N,S,S] f32, center [N,2,S,S] f32, int_boxes [N,4] i32 (x1,y1,x2,y2 clipped to the image), all on the device"""
    import torch
    from . import _lib as L
    from .ops import _need_gpu, _p, _stream
    _need_gpu(sdf, center, int_boxes, select)
    assert sdf.dtype == torch.float32 and center.dtype == torch.float32 and int_boxes.dtype == torch.int32 and select.dtype == torch.int64
    sdf, center, int_boxes, select = sdf.contiguous(), center.contiguous(), int_boxes.contiguous(), select.contiguous()
    K, S = len(select), sdf.shape[-1]
    if K == 0:
        return []

    def launch(sizes, offsets, chars, cap):
        L.check(L.lib().umr_mask_paste_rle(_p(sdf), _p(center), _p(int_boxes), _p(select), K, S, H, W, _p(sizes), _p(offsets), _p(chars), cap,
                                           _stream()), "umr_mask_paste_rle")
    return _two_pass(launch, K, H, W, sdf.device)


POLY_SORT_LDS_KEYS = 4096      # csrc/poly_rle.hip POLY_LDS_KEYS: crossing lists up to this length are sorted in LDS, longer ones in memory


def _poly_tables(polys, sizes):
    """the packed upload of `from_polygons`: float64 coordinates, then int64 polygon offsets (in vertices), annotation polygon ranges,
    annotation sizes and the crossing slices (prefix sums of the bound sum over edges of min(dx, W) + 1 -- an edge's u is monotone, so
    it steps over every column line at most once, and once more where it joins the previous edge).  Returns (host u8 array, byte
    offsets of the five tables, V, NP, NA, C)."""
    flat = [c for mine in polys for c in mine]
    NA, NP = len(polys), len(flat)
    nv = np.array([c.size // 2 for c in flat], dtype=np.int64)
    poly_off = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
    ann_poly = np.concatenate([[0], np.cumsum([len(mine) for mine in polys])]).astype(np.int64)
    ann_size = np.array(sizes, dtype=np.int64).reshape(NA, 2)
    xy = np.concatenate(flat + [np.zeros(2)]).astype(np.float64)             # never empty
    V = int(poly_off[-1])
    bound = np.zeros(NP, dtype=np.int64)
    if NP:
        x = np.trunc(POLY_SCALE * xy[0:2 * V:2] + .5).astype(np.int64)       # step 1's formula
        nxt = np.arange(V) + 1
        nxt[poly_off[1:] - 1] = poly_off[:-1]                                # the ring closes on the polygon's first vertex
        w_of_poly = np.repeat(ann_size[:, 1], np.diff(ann_poly))
        per_edge = np.minimum(np.abs(x[nxt] - x), np.repeat(w_of_poly, nv)) + 1
        bound = np.add.reduceat(per_edge, poly_off[:-1])
    cross_off = np.concatenate([[0], np.cumsum(bound)]).astype(np.int64)
    tables = [xy.view(np.uint8), poly_off.view(np.uint8), ann_poly.view(np.uint8), ann_size.reshape(-1).view(np.uint8), cross_off.view(np.uint8)]
    offs = np.concatenate([[0], np.cumsum([t.size for t in tables])])[:-1]
    return np.concatenate(tables), [int(o) for o in offs], V, NP, NA, int(cross_off[-1])


def from_polygons(segmentations, sizes, device="cuda", phase_ms=None):
    """pycocotools' annToRLE for polygon segmentations, on the device (csrc/poly_rle.hip).  segmentations[i]: a COCO polygon
    `segmentation`, i.e. a list of flat [x0, y0, x1, y1, ...] lists (the annotation's mask is the union of its polygons); sizes: one
    (H, W) or one per segmentation.  Returns the records {'size': [H, W], 'counts': str}, byte for byte what `from_polygons_numpy`
    gives.  One host-to-device copy carries the coordinates and the tables, two small reads come back (the sizes, then the packed
    strings).  A coordinate list of odd length, a non-finite coordinate, one beyond 2^20 in magnitude and H*W >= 2^31 raise
    ValueError before any launch.  phase_ms: a dict that receives the device time of the three phases (tools/polygon_rle_bench.py)."""
    import torch
    polys, sizes = _check_polygons(segmentations, sizes, "from_polygons")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("unmore_amd.rle.from_polygons runs on the MI355X only (no CPU fallback); from_polygons_numpy restates it on the host")
    if not polys:
        return []
    from . import _lib as L
    from ._tables import workspace
    from .ops import _p, _stream
    host, (o_xy, o_po, o_ap, o_as, o_co), V, NP, NA, C = _poly_tables(polys, sizes)
    if C >= 1 << 31 or V >= 1 << 31:
        raise ValueError("from_polygons: more than 2^31 vertices or possible crossings in one call; split the batch")
    vp = ctypes.c_void_p
    with torch.cuda.device(device):
        buf = torch.from_numpy(host).to(device)
        nbytes = L.lib().umr_poly_rle_workspace(V, NP, NA, C)
        ws = workspace(nbytes, device)
        base = buf.data_ptr()

        def run(phases, sizes_t, offsets, chars, cap):
            L.check(L.lib().umr_poly_rle(vp(base + o_xy), vp(base + o_po), vp(base + o_ap), vp(base + o_as), vp(base + o_co), V, NP, NA, C, phases,
                                         _p(sizes_t), _p(offsets), _p(chars), cap, vp(ws.data_ptr()), nbytes, _stream()), "umr_poly_rle")

        def launch(sizes_t, offsets, chars, cap):
            if chars is not None:                                          # the write pass reads what the measure pass left in the workspace
                if phase_ms is None:
                    return run(4, sizes_t, offsets, chars, cap)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                run(4, sizes_t, offsets, chars, cap)
                t1.record()
                t1.synchronize()
                phase_ms["characters"] += t0.elapsed_time(t1)             # measure pass + write pass
                return None
            if phase_ms is None:
                return run(7, sizes_t, offsets, chars, cap)
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for i, phases in enumerate((1, 2, 4)):
                marks[i].record()
                run(phases, sizes_t, offsets, chars, cap)
            marks[3].record()
            marks[3].synchronize()
            phase_ms.update({k: marks[i].elapsed_time(marks[i + 1]) for i, k in enumerate(("generate", "sort", "characters"))})
        out = _two_pass(launch, NA, 0, 0, device)
    for rec, (H, W) in zip(out, sizes):
        rec["size"] = [H, W]
    return out


# ---------------------------------------------------------------------------------------------------------------- strings -> masks
_STATUS_BITS = ((1, "a character outside the format or a string that stops inside a number"),
                (2, "a number of more than 7 characters or a count outside [0, H*W]"),
                (4, "counts that do not sum to H*W"),
                (8, "a table entry out of range"))


def _as_record(rec, k, what):
    """a segmentation -> (H, W, counts as bytes); uncompressed count lists are converted with counts_to_string"""
    if isinstance(rec, (list, tuple)):
        raise ValueError(f"{what}: record {k} is a polygon segmentation; only run-length records {{'size', 'counts'}} are decoded")
    if not isinstance(rec, dict) or "size" not in rec or "counts" not in rec:
        raise ValueError(f"{what}: record {k} is not a run-length record {{'size': [H, W], 'counts': str | bytes | list}}")
    size = rec["size"]
    if len(size) != 2:
        raise ValueError(f"{what}: record {k}: size is [H, W]")
    H, W = int(size[0]), int(size[1])
    if H <= 0 or W <= 0 or H * W >= 1 << 31:
        raise ValueError(f"{what}: record {k}: size {[H, W]} must be positive with H*W < 2^31")
    c = rec["counts"]
    if isinstance(c, str):
        c = c.encode("ascii")
    elif not isinstance(c, (bytes, bytearray)):
        c = counts_to_string(c).encode("ascii")
    return H, W, bytes(c)


def as_record(rec):
    """the string form of a run-length segmentation, as `decode` / `largest_component` read every record they are given:
    {'size': [H, W], 'counts': str}; bytes are decoded, an uncompressed count list is converted with counts_to_string; a polygon
    raises ValueError.  decode_numpy(as_record(r)) is the host's answer for any record the device calls accept."""
    H, W, c = _as_record(rec, 0, "as_record")
    return {"size": [H, W], "counts": c.decode("ascii")}


def _prepare(records, groups, mode, what):
    """host-side checks and tables, before any launch: (recs, sizes [G] of (H, W), group_start [G+1])"""
    recs = [_as_record(r, k, what) for k, r in enumerate(records)]
    K = len(recs)
    if groups is None:
        groups = [(1, (h, w)) for h, w, _ in recs]
    starts, sizes = [0], []
    for g, (n, size) in enumerate(groups):
        n, H, W = int(n), int(size[0]), int(size[1])
        if n < 0 or H <= 0 or W <= 0 or H * W >= 1 << 31:
            raise ValueError(f"{what}: group {g}: a record count >= 0 and a positive size with H*W < 2^31 expected")
        if mode == 1 and n != 1:
            raise ValueError(f"{what}: group {g} holds {n} records; the largest component is taken of exactly one")
        if starts[-1] + n > K:
            raise ValueError(f"{what}: the groups take more than the {K} records given")
        for k in range(starts[-1], starts[-1] + n):
            if (recs[k][0], recs[k][1]) != (H, W):
                raise ValueError(f"{what}: record {k} has size {[recs[k][0], recs[k][1]]}, its group {g} has {[H, W]}")
        starts.append(starts[-1] + n)
        sizes.append((H, W))
    if starts[-1] != K:
        raise ValueError(f"{what}: the groups take {starts[-1]} of the {K} records given")
    return recs, sizes, starts


def _decode_call(records, groups, mode, device, what):
    import torch
    recs, sizes, starts = _prepare(records, groups, mode, what)
    K, G = len(recs), len(sizes)
    if G == 0:
        return [], None
    from . import _lib as L
    from ._tables import workspace
    from .ops import _stream
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"unmore_amd.rle.{what} runs on the MI355X only (no CPU fallback); decode_numpy restates the format on the host")
    # ---- every table and the characters in one buffer, one host-to-device copy
    nchars = np.array([len(c) for _, _, c in recs], dtype=np.int64)
    char_offsets = np.concatenate([[0], np.cumsum(nchars)]).astype(np.int64)
    total_chars = int(char_offsets[-1])
    out_desc = np.zeros((G, 3), dtype=np.int64)
    off = 0
    for g, (h, w) in enumerate(sizes):
        out_desc[g] = (h, w, off)
        off += (h * w + 15) & ~15                                            # every mask starts on a 16-byte boundary
    out_bytes = off
    seg_offsets = np.zeros(G + 1, dtype=np.int64)
    if mode == 1:
        seg_offsets[1:] = np.cumsum(nchars // 2 + 1 + np.array([w for _, w in sizes], dtype=np.int64))
    total_segments = int(seg_offsets[-1])
    gs = np.zeros((G + 2) & ~1, dtype=np.int32)
    gs[:G + 1] = starts
    tables = np.concatenate([char_offsets, out_desc.reshape(-1), seg_offsets, gs.view(np.int64)])
    o_desc, o_seg, o_gs, o_chars = (K + 1) * 8, (K + 1 + 3 * G) * 8, (K + 1 + 3 * G + G + 1) * 8, tables.size * 8
    host = np.concatenate([tables.view(np.uint8), np.frombuffer(b"".join(c for _, _, c in recs), dtype=np.uint8)])
    with torch.cuda.device(device):
        buf = torch.from_numpy(host).to(device)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=device)
        status = torch.empty(max(K, 1), dtype=torch.int32, device=device)
        info = torch.empty((G, 2), dtype=torch.int32, device=device) if mode == 1 else None
        nbytes = L.lib().umr_rle_decode_workspace(K, total_chars, total_segments, mode)
        ws = workspace(nbytes, device)
        base = buf.data_ptr()
        vp = ctypes.c_void_p
        L.check(L.lib().umr_rle_decode(vp(base + o_chars), vp(base), K, total_chars, vp(base + o_desc), vp(base + o_gs), vp(base + o_seg), G,
                                       max(h * w for h, w in sizes), total_segments, vp(out.data_ptr()), out_bytes, 255, mode,
                                       vp(status.data_ptr()), vp(info.data_ptr()) if info is not None else None, vp(ws.data_ptr()), nbytes,
                                       _stream()), "umr_rle_decode")
        st = status[:K].cpu().numpy() if K else np.zeros(0, np.int32)         # the call's only synchronisation
    masks = [out[int(o):int(o) + h * w].view(h, w) for (h, w), o in zip(sizes, out_desc[:, 2])]
    bad = np.flatnonzero(st)
    if bad.size:
        k = int(bad[0])
        why = "; ".join(t for b, t in _STATUS_BITS if int(st[k]) & b)
        more = f" (also malformed: records {', '.join(str(int(b)) for b in bad[1:])})" if bad.size > 1 else ""
        err = ValueError(f"{what}: record {k} is not a run-length string of a {recs[k][0]}x{recs[k][1]} mask: {why}{more}")
        err.status, err.masks, err.info = st, masks, info     # what the well-formed records gave; a malformed one contributed nothing
        raise err
    return masks, info


def decode(records, groups=None, device="cuda"):
    """run-length records -> list of [h, w] u8 device tensors holding 0 / 255 (views into one packed buffer).  records: a list of
    {'size': [H, W], 'counts': str | bytes} or of uncompressed records whose counts are a list (converted with counts_to_string);
    polygon segmentations raise ValueError.  groups=None: one mask per record.  Otherwise a list of (n, (H, W)): output g is the
    union (OR) of the next n records, all of size (H, W); n = 0 gives an all-zero mask.  The strings are parsed on the device
    (csrc/rle_decode.hip); one host-to-device copy carries the tables and the characters; the status words are read back once after
    the launches -- the call's only synchronisation -- and a malformed string raises ValueError naming its record.  That error
    carries what the call did make: `.status` (int32 numpy array, one word per record, the bits of umr_rle_decode), `.masks` (the list
    the call would have returned; a malformed record contributed nothing to its mask) and `.info` (None here).  Argument errors
    (non-positive sizes, mixed sizes inside a group) are raised before any launch and carry none of these."""
    return _decode_call(records, groups, 0, device, "decode")[0]


def largest_component(records, device="cuda"):
    """per record the largest 4-connected component of its mask, as utils/preprocess_votecut.py:88-92 takes it
    (cv2.connectedComponentsWithStats(mask, 4), np.argmax of the areas: ties go to the component whose first pixel in raster order
    comes first).  Returns (masks, info): masks as `decode` returns them; info int32 [K, 2] on the device = (number of components,
    area of the kept one), (0, 0) for an empty mask.  Runs are labelled, not pixels: see csrc/rle_decode.hip.  A malformed string
    raises ValueError as in `decode`, with `.status`, `.masks` (all zero for the malformed record) and `.info` attached."""
    masks, info = _decode_call(records, None, 1, device, "largest_component")
    if info is None:
        import torch
        info = torch.empty((0, 2), dtype=torch.int32, device=device)
    return masks, info
