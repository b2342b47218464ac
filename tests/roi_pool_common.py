"""Comparators for unmore_amd.roi_pool (shared by the CPU and GPU tests and tools/roi_pool_bench.py), written from Detectron2's and
torchvision's published definitions.

axis_samples / axis_matrix: the samples of one axis of one box under torchvision's roi_align(aligned=True) and their summed tap weights
A [P, size] -- ROIAlign is separable, out[c] = Ay F[c] Ax^T / count.
roi_align_np / roi_align_adjoint_np: that form and its adjoint Ay^T G Ax / count in float64 (of the float32 inputs).
roi_align_f32_samples: one box in float32, sample by sample in torchvision's order (iy outer, ix inner, one rounding per operation) --
what the original runs, the yardstick for the tolerances.
assign_levels: Detectron2's assign_boxes_to_levels as its float32 torch sequence on the CPU.
pooler_np: the ROIPooler -- levels, per-level roi_align, scatter into input order.
level_maps / edge_case_boxes / recipe_batch: seeded inputs."""
import numpy as np
import torch

MAX_COORD = float(1 << 20)


def bad_boxes(boxes):
    """what the device refuses: a coordinate that is not finite or beyond +-2^20"""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(boxes) <= MAX_COORD).all(1)


def axis_samples(lo, hi, P, size, scale=1.0, sampling_ratio=0, dt=np.float64):
    """(coordinate, valid, low, high, l, h) as [P, grid] arrays of one axis of one box, arithmetic in dt on the float32 inputs; None for
    roi <= 0 or an empty grid.  start = lo * scale - .5; roi = (hi * scale - .5) - start; bin = roi / P; grid = sampling_ratio or
    ceil(bin); coordinate(p, i) = (start + p * bin) + ((i + .5) * bin) / grid; valid inside [-1, size]; then clamped to [0, size - 1]."""
    lo, hi, scale, half = dt(np.float32(lo)), dt(np.float32(hi)), dt(np.float32(scale)), dt(0.5)
    start = dt(dt(lo * scale) - half)
    roi = dt(dt(dt(hi * scale) - half) - start)
    if not roi > 0:
        return None
    bin_ = dt(roi / dt(P))
    grid = int(sampling_ratio) if sampling_ratio > 0 else int(np.ceil(bin_))
    if grid < 1:
        return None
    p = np.arange(P, dtype=dt)[:, None]
    i = np.arange(grid, dtype=dt)[None, :]
    coord = (start + p * bin_) + ((i + half) * bin_) / dt(grid)
    assert coord.dtype == dt
    valid = (coord >= -1) & (coord <= size)
    c = np.where(coord <= 0, dt(0), coord)
    low = np.where(valid, c, 0).astype(np.int64)
    top = low >= size - 1
    low = np.where(top, size - 1, low)
    high = np.where(top, size - 1, low + 1)
    c = np.where(top, low.astype(dt), c)
    l = (c - low.astype(dt)).astype(dt)
    h = (dt(1) - l).astype(dt)
    return coord, valid, low, high, np.where(valid, l, dt(0)), np.where(valid, h, dt(0))


def axis_matrix(lo, hi, P, size, scale=1.0, sampling_ratio=0, dt=np.float64):
    """(A [P, size] in dt, grid): A[p, t] = the summed weight of tap t over the samples of bin p; (zeros, 0) without samples"""
    A = np.zeros((P, size), dtype=dt)
    s = axis_samples(lo, hi, P, size, scale, sampling_ratio, dt)
    if s is None:
        return A, 0
    _, valid, low, high, l, h = s
    rows = np.broadcast_to(np.arange(P)[:, None], low.shape)
    np.add.at(A, (rows[valid], low[valid]), h[valid])
    np.add.at(A, (rows[valid], high[valid]), l[valid])
    return A, low.shape[1]


def axis_touch(lo, hi, P, size, scale=1.0, sampling_ratio=0):
    """T float64 [P, size]: the number of valid samples of bin p that have tap t among low - 1 .. high + 1 -- the taps a sample's weight
    can reach when its float32 coordinate is off by a little"""
    T = np.zeros((P, size), dtype=np.float64)
    s = axis_samples(lo, hi, P, size, scale, sampling_ratio, np.float64)
    if s is None:
        return T
    _, valid, low, high, _, _ = s
    rows = np.broadcast_to(np.arange(P)[:, None], low.shape)
    for tap in (low - 1, low, high, high + 1):
        ok = valid & (tap >= 0) & (tap < size)
        np.add.at(T, (rows[ok], tap[ok]), 1.0)
    return T


def coord_error(lo, hi, scale):
    """A bound on |float32 coordinate - float64 coordinate| of one axis: the expression ((lo s - .5) + p bin) + ((i + .5) bin) / grid has
    eight roundings on the way (lo s, - .5, hi s, - .5, the difference, / P, p bin, the sum; the last term is below one bin and its
    roundings are below one of the others'), none of a value above M = max(|start|, |start + roi|) + 1: 8 * 2^-24 * M"""
    a, b = abs(float(np.float32(lo)) * scale - 0.5), abs(float(np.float32(hi)) * scale - 0.5)
    return 8.0 * 2.0 ** -24 * (max(a, b) + 1.0)


def _rois(rois):
    rois = np.asarray(rois, dtype=np.float32).reshape(-1, 5)
    return rois, bad_boxes(rois[:, 1:])


def _span(A):
    """the slice of columns of A that hold a weight"""
    cols = np.nonzero(A.any(0))[0]
    return slice(int(cols[0]), int(cols[-1]) + 1) if cols.size else slice(0, 0)


def _matrices(roi, P, H, W, scale, sampling_ratio):
    Ay, gh = axis_matrix(roi[2], roi[4], P, H, scale, sampling_ratio)
    Ax, gw = axis_matrix(roi[1], roi[3], P, W, scale, sampling_ratio)
    return Ay, Ax, gh * gw


def roi_align_np(features, rois, P, scale=1.0, sampling_ratio=0):
    """float64 [R,C,P,P] of features [N,C,H,W] and rois [R,5] = (image, x1, y1, x2, y2): Ay F Ax^T / count; a refused roi gives zeros"""
    F = np.asarray(features)
    N, C, H, W = F.shape
    rois, bad = _rois(rois)
    out = np.zeros((rois.shape[0], C, P, P), dtype=np.float64)
    for r, roi in enumerate(rois):
        if bad[r] or not (0 <= roi[0] < N and roi[0] == np.floor(roi[0])):
            continue
        Ay, Ax, count = _matrices(roi, P, H, W, scale, sampling_ratio)
        if count:
            ys, xs = _span(Ay), _span(Ax)                                # the footprint: the product over the rest of the map is zero
            out[r] = np.einsum("py,cyx,qx->cpq", Ay[:, ys], F[int(roi[0]), :, ys, xs].astype(np.float64), Ax[:, xs], optimize=True) / count
    return out


def roi_align_abs_np(features, rois, P, scale=1.0, sampling_ratio=0):
    """the same over |features|: the magnitude the rounding allowances scale with (the weights are not negative)"""
    return roi_align_np(np.abs(np.asarray(features, dtype=np.float64)), rois, P, scale, sampling_ratio)


def roi_align_adjoint_np(grad_out, rois, shape, P, scale=1.0, sampling_ratio=0):
    """float64 [N,C,H,W]: the adjoint, sum over the rois of Ay^T G Ax / count"""
    G = np.asarray(grad_out)
    N, C, H, W = shape
    rois, bad = _rois(rois)
    grad = np.zeros(shape, dtype=np.float64)
    for r, roi in enumerate(rois):
        if bad[r] or not (0 <= roi[0] < N and roi[0] == np.floor(roi[0])):
            continue
        Ay, Ax, count = _matrices(roi, P, H, W, scale, sampling_ratio)
        if count:
            ys, xs = _span(Ay), _span(Ax)
            grad[int(roi[0]), :, ys, xs] += np.einsum("py,cpq,qx->cyx", Ay[:, ys], G[r].astype(np.float64), Ax[:, xs], optimize=True) / count
    return grad


U32 = 2.0 ** -24


def _valid_rois(rois, N):
    rois, bad = _rois(rois)
    return rois, [r for r, roi in enumerate(rois) if not bad[r] and 0 <= roi[0] < N and roi[0] == np.floor(roi[0])]


def forward_allowance(features, rois, P, scale=1.0, sampling_ratio=0):
    """Bound (a) of the GPU tests on |device - float64| per output element, from the kernel's order of operations (csrc/roi_pool.hip):
    a table entry is a float32 sum of at most grid weights, each 1 - l with one rounding (<= grid + 1 roundings); the kernel adds
    sum_x Ax F over the n_x taps of the bin (a product and an add each: <= n_x + 1), multiplies by Ay (1), adds the n_y rows (n_y) and
    divides (1).  To first order every product Ay Ax F carries at most k = grid_h + grid_w + n_y + n_x + 8 relative errors of 2^-24
    (the 8: the five single operations and the second-order terms), so the sum is off by at most k 2^-24 (Ay |F| Ax^T / count).
    The weight-rounding term: a float32 sample coordinate is off by at most d = coord_error(), which moves at most d of the sample's
    weight between two taps per axis, so a sample and with it the mean of the samples moves by at most 2 (d_y + d_x) max|F[n, c]|."""
    F = np.abs(np.asarray(features, dtype=np.float64))
    N, C, H, W = F.shape
    rois, valid = _valid_rois(rois, N)
    out = np.zeros((rois.shape[0], C, P, P), dtype=np.float64)
    for r in valid:
        roi = rois[r]
        Ay, Ax, count = _matrices(roi, P, H, W, scale, sampling_ratio)
        if not count:
            continue
        gh, gw = axis_matrix(roi[2], roi[4], P, H, scale, sampling_ratio)[1], axis_matrix(roi[1], roi[3], P, W, scale, sampling_ratio)[1]
        k = gh + gw + int((Ay != 0).sum(1).max()) + int((Ax != 0).sum(1).max()) + 8
        d = coord_error(roi[2], roi[4], scale) + coord_error(roi[1], roi[3], scale)
        n = int(roi[0])
        out[r] = k * U32 * np.einsum("py,cyx,qx->cpq", Ay, F[n], Ax) / count + 2 * d * F[n].max(axis=(1, 2))[:, None, None]
    return out


def backward_allowance(grad_out, rois, shape, P, scale=1.0, sampling_ratio=0):
    """Bound (a) on |device - float64| per element of the feature gradient.  The kernel adds ((Ay[ph,y] Ax[pw,x]) / count) g to the
    pixel's running sum, one term per bin that touches the pixel, box after box: a term carries the roundings of its two table entries
    (<= grid_h + 1, grid_w + 1), of the product, the division and the product with g, and of every add that follows it, at most the
    S = sum over the image's boxes of h_y h_x adds a pixel can receive (h: the most bins of a box that share one tap).  So every term
    is off by at most k = grid_h + grid_w + 8 + S relative errors of 2^-24, on Ay^T |G_r| Ax / count.  The weight-rounding term: the
    weights of tap y over the bins change by at most d_y T_y[y], T the number of samples that can reach the tap (axis_touch), so the
    pixel moves by at most max|G_r[c]| (d_y T_y[y] sum_pw Ax[pw,x] + d_x T_x[x] sum_ph Ay[ph,y]) / count."""
    G = np.abs(np.asarray(grad_out, dtype=np.float64))
    N, C, H, W = shape
    rois, valid = _valid_rois(rois, N)
    out = np.zeros(shape, dtype=np.float64)
    mats, adds = {}, np.zeros(N, dtype=np.int64)
    for r in valid:
        roi = rois[r]
        Ay, gh = axis_matrix(roi[2], roi[4], P, H, scale, sampling_ratio)
        Ax, gw = axis_matrix(roi[1], roi[3], P, W, scale, sampling_ratio)
        if gh * gw:
            mats[r] = (Ay, Ax, gh, gw)
            adds[int(roi[0])] += int((Ay != 0).sum(0).max()) * int((Ax != 0).sum(0).max())
    for r, (Ay, Ax, gh, gw) in mats.items():
        roi, count = rois[r], gh * gw
        n = int(roi[0])
        k = gh + gw + 8 + int(adds[n])
        Ty, Tx = axis_touch(roi[2], roi[4], P, H, scale, sampling_ratio), axis_touch(roi[1], roi[3], P, W, scale, sampling_ratio)
        dy, dx = coord_error(roi[2], roi[4], scale), coord_error(roi[1], roi[3], scale)
        moved = dy * np.outer(Ty.sum(0), Ax.sum(0)) + dx * np.outer(Ay.sum(0), Tx.sum(0))
        out[n] += k * U32 * np.einsum("py,cpq,qx->cyx", Ay, G[r], Ax) / count + G[r].max(axis=(1, 2))[:, None, None] * moved[None] / count
    return out


def tap_support(rois, shape, P, scale=1.0, sampling_ratio=0):
    """bool [N,H,W]: the pixels a tap of some roi can land on (axis_touch: the taps and their neighbours)"""
    N, _, H, W = shape
    rois, valid = _valid_rois(rois, N)
    out = np.zeros((N, H, W), dtype=bool)
    for r in valid:
        roi = rois[r]
        Ty, Tx = axis_touch(roi[2], roi[4], P, H, scale, sampling_ratio), axis_touch(roi[1], roi[3], P, W, scale, sampling_ratio)
        out[int(roi[0])] |= np.outer(Ty.sum(0) > 0, Tx.sum(0) > 0)
    return out


def roi_align_adjoint_f32_np(grad_out, rois, shape, P, scale=1.0, sampling_ratio=0):
    """The adjoint with float32 samples, weights and sums (one float32 einsum per box, boxes added in order): the backward's counterpart
    of roi_align_f32_np -- torchvision's own backward adds its taps with atomics, in no fixed order."""
    G = np.asarray(grad_out, dtype=np.float32)
    N, C, H, W = shape
    rois, valid = _valid_rois(rois, N)
    grad = np.zeros(shape, dtype=np.float32)
    for r in valid:
        roi = rois[r]
        Ay, gh = axis_matrix(roi[2], roi[4], P, H, scale, sampling_ratio, np.float32)
        Ax, gw = axis_matrix(roi[1], roi[3], P, W, scale, sampling_ratio, np.float32)
        if gh * gw:
            grad[int(roi[0])] += np.einsum("py,cpq,qx->cyx", Ay, G[r], Ax) / np.float32(gh * gw)
    return grad


def roi_align_f32_samples(feature, roi, P, scale=1.0, sampling_ratio=0):
    """float32 [C,P,P] of one map [C,H,W] and one box (x1, y1, x2, y2), as torchvision's kernel computes it: per bin the samples iy outer,
    ix inner, val = w1 v1 + w2 v2 + w3 v3 + w4 v4 with w1 = hy hx, ..., one float32 rounding per operation, then / count"""
    f = np.asarray(feature, dtype=np.float32)
    C, H, W = f.shape
    out = np.zeros((C, P, P), dtype=np.float32)
    if bad_boxes(roi)[0]:
        return out
    sy = axis_samples(roi[1], roi[3], P, H, scale, sampling_ratio, np.float32)
    sx = axis_samples(roi[0], roi[2], P, W, scale, sampling_ratio, np.float32)
    if sy is None or sx is None:
        return out
    _, vy, yl, yh, ly, hy = sy
    _, vx, xl, xh, lx, hx = sx
    gh, gw = yl.shape[1], xl.shape[1]
    for iy in range(gh):
        for ix in range(gw):
            a, b = (slice(None), iy), (slice(None), ix)
            w1, w2 = np.outer(hy[a], hx[b]), np.outer(hy[a], lx[b])
            w3, w4 = np.outer(ly[a], hx[b]), np.outer(ly[a], lx[b])
            v1, v2 = f[:, yl[a][:, None], xl[b][None, :]], f[:, yl[a][:, None], xh[b][None, :]]
            v3, v4 = f[:, yh[a][:, None], xl[b][None, :]], f[:, yh[a][:, None], xh[b][None, :]]
            val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4
            assert val.dtype == np.float32
            out += np.where(np.outer(vy[a], vx[b]), val, np.float32(0))
    return out / np.float32(max(gh * gw, 1))


def roi_align_f32_np(features, rois, P, scale=1.0, sampling_ratio=0):
    """roi_align_f32_samples over features [N,C,H,W] and rois [R,5]: float32 [R,C,P,P]"""
    f = np.asarray(features, dtype=np.float32)
    rois, bad = _rois(rois)
    out = np.zeros((rois.shape[0], f.shape[1], P, P), dtype=np.float32)
    for r, roi in enumerate(rois):
        if not bad[r] and 0 <= roi[0] < f.shape[0] and roi[0] == np.floor(roi[0]):
            out[r] = roi_align_f32_samples(f[int(roi[0])], roi[1:], P, scale, sampling_ratio)
    return out


def sample_margin(rois, P, H, W, scale=1.0, sampling_ratio=0):
    """The input condition of the GPU tests, on the float64 samples: (the least distance of any sample coordinate from -1 or from the
    size -- the rule's only discontinuities --, whether float32 and float64 agree on every adaptive grid)"""
    rois, bad = _rois(rois)
    margin, same = np.inf, True
    for r, roi in enumerate(rois):
        if bad[r]:
            continue
        for lo, hi, size in ((roi[2], roi[4], H), (roi[1], roi[3], W)):
            s64 = axis_samples(lo, hi, P, size, scale, sampling_ratio, np.float64)
            s32 = axis_samples(lo, hi, P, size, scale, sampling_ratio, np.float32)
            same = same and (s64 is None) == (s32 is None) and (s64 is None or s64[0].shape == s32[0].shape)
            if s64 is not None:
                margin = min(margin, np.abs(s64[0] + 1).min(), np.abs(s64[0] - size).min())
    return margin, same


def assign_levels(boxes, min_level, max_level, canonical_box_size=224, canonical_level=4):
    """int64 [R]: Detectron2's float32 torch sequence on the CPU -- sqrt(area), floor(canonical_level + log2(s / size + 1e-8)), clamp,
    minus min_level; a refused box and a NaN level (negative area) give level 0, the module's documented departures"""
    b = torch.as_tensor(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    sizes = torch.sqrt(area)
    lv = torch.floor(canonical_level + torch.log2(sizes / canonical_box_size + 1e-8))
    assert lv.dtype == torch.float32
    lv = torch.where(torch.isnan(lv), torch.full_like(lv, float(min_level)), lv)
    lv = torch.clamp(lv, min=min_level, max=max_level).to(torch.int64) - min_level
    lv[torch.as_tensor(bad_boxes(boxes))] = 0
    return lv.numpy()


def pooler_rois(box_lists):
    """[R,5] float32 rois of the boxes per image, Detectron2's convert_boxes_to_pooler_format"""
    rows = [np.concatenate([np.full((len(b), 1), k, dtype=np.float32), np.asarray(b, dtype=np.float32).reshape(-1, 4)], 1)
            for k, b in enumerate(box_lists)]
    return np.concatenate(rows) if rows else np.zeros((0, 5), dtype=np.float32)


def pooler_np(features, box_lists, P, scales, sampling_ratio=0, canonical_box_size=224, canonical_level=4, levels=None):
    """float64 [sum R_k, C, P, P]: the ROIPooler over the level maps features[l] [N,C,H_l,W_l]; `levels` overrides the assignment"""
    rois = pooler_rois(box_lists)
    min_level, max_level = int(round(-np.log2(scales[0]))), int(round(-np.log2(scales[-1])))
    if levels is None:
        levels = assign_levels(rois[:, 1:], min_level, max_level, canonical_box_size, canonical_level) if len(scales) > 1 \
            else np.zeros(len(rois), dtype=np.int64)
    out = np.zeros((len(rois), features[0].shape[1], P, P), dtype=np.float64)
    for l, (f, s) in enumerate(zip(features, scales)):
        pick = np.nonzero(levels == l)[0]
        if pick.size:
            out[pick] = roi_align_np(f, rois[pick], P, s, sampling_ratio)
    return out


def pooler_adjoint_np(grad_out, features_shapes, box_lists, P, scales, sampling_ratio=0, levels=None):
    """the adjoint of pooler_np: one float64 gradient per level"""
    rois = pooler_rois(box_lists)
    min_level, max_level = int(round(-np.log2(scales[0]))), int(round(-np.log2(scales[-1])))
    if levels is None:
        levels = assign_levels(rois[:, 1:], min_level, max_level) if len(scales) > 1 else np.zeros(len(rois), dtype=np.int64)
    G = np.asarray(grad_out, dtype=np.float64)
    grads = []
    for l, (shape, s) in enumerate(zip(features_shapes, scales)):
        pick = np.nonzero(levels == l)[0]
        grads.append(roi_align_adjoint_np(G[pick], rois[pick], shape, P, s, sampling_ratio))
    return grads


# ---- seeded inputs
FRAME = (128, 192)
STRIDES = (4, 8, 16, 32)


def level_maps(rng, N, C, frame=FRAME, strides=STRIDES):
    """float32 maps [N,C,H/s,W/s] per stride, standard normal"""
    return [rng.standard_normal((N, C, frame[0] // s, frame[1] // s)).astype(np.float32) for s in strides]


def edge_case_boxes(seed=0, frame=FRAME, copies=50):
    """The GPU tests' boxes for one image of `frame` under levels p2..p5 (canonical size 224 at level 4, so the level boundaries are
    the box sides 112 / 224 / 448; the boxes of the coarser levels reach far beyond the small frame).  A dict of name -> float32 [k,4];
    `all` concatenates them in a fixed order with `copies` copies of one box at the end."""
    rng = np.random.RandomState(seed)
    H, W = frame
    j = lambda: rng.uniform(0.13, 0.87)                                   # noqa: E731  a fractional offset
    out = {}
    straddle = []
    for side in (112, 224, 448):                                          # just under, exactly on, just over each boundary
        for d in (-0.5, 0.0, 0.5):
            x, y = W // 2 - side // 2 + rng.randint(-10, 11), H // 2 - side // 2 + rng.randint(-10, 11)    # integers: the side is exact
            straddle.append([x, y, x + side + d, y + side + d])
    out["straddle"] = straddle
    out["beyond"] = [[-3.3 - j(), 20 + j(), 40 + j(), 70 + j()], [150 + j(), 30 + j(), W + 2.4 + j(), 90 + j()],
                     [30 + j(), -2.2 - j(), 90 + j(), 50 + j()], [60 + j(), 80 + j(), 130 + j(), H + 1.6 + j()]]
    out["outside"] = [[W + 9.3, 10.2, W + 40.6, 60.7]]
    out["zero_width"] = [[50.4, 20.3, 50.4, 60.9]]
    out["tiny"] = [[70.21, 40.37, 72.93, 43.11]]                          # under one pixel of the finest map
    out["huge"] = [[-300.3, -200.7, 500.9, 330.2]]                        # side 650: the coarsest level
    out["nan"] = [[10.0, np.nan, 50.0, 60.0]]
    n_random = 70 - copies - sum(len(v) for v in out.values())
    rand = []
    for _ in range(max(n_random, 0)):
        w, h = rng.uniform(4, 120), rng.uniform(4, 100)
        x, y = rng.uniform(-2, W - w + 2), rng.uniform(-2, H - h + 2)
        rand.append([x, y, x + w, y + h])
    out["random"] = rand
    out["copies"] = [[33.37, 11.61, 151.83, 125.29]] * copies                # side 116: the second level
    out = {k: np.asarray(v, dtype=np.float32).reshape(-1, 4) for k, v in out.items()}
    out["all"] = np.concatenate([out[k] for k in ("straddle", "beyond", "outside", "zero_width", "tiny", "huge", "nan", "random", "copies")])
    return out


def recipe_batch(seed, images=16, per_image=512, frame=(800, 1216)):
    """tools/roi_pool_bench.py's proposals: drawn as tools/box_loss_bench.py draws them (box_loss_common.ragged_batch)"""
    from box_loss_common import ragged_batch
    batch = ragged_batch(seed, [per_image] * images, [20] * images, [frame] * images, box_scale=0.3)
    return [im["proposal_boxes"].astype(np.float32) for im in batch]
