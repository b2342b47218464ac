"""The proposal step of the stage-3 detector's RPN on the device: from the RPN head's raw outputs on every pyramid level to the
proposals per image that the ROI heads consume.  The reference calls it on every training step and every inference image
(cad/modeling/meta_arch/rcnn.py:165, 213, 333: self.proposal_generator(images, features, ...)); it is Detectron2's
RPN.predict_proposals -> _decode_proposals + find_top_rpn_proposals with DefaultAnchorGenerator's anchors.

  cell_anchors     DefaultAnchorGenerator.generate_cell_anchors per level (host)
  grid_anchors     the anchors of whole level maps as tensors, for callers and tests -- the kernels never read an anchor tensor
  rpn_proposals    per (image, level) top-k of the logits read in place, decode of the selected anchors only, clip, drop of non-finite
                   and empty boxes, NMS per level, merge and truncation: five launches for the whole batch (csrc/rpn.hip), one read of
                   the counts in the list form and none in the padded form

The steps, in order (tests/rpn_common.py restates them in NumPy float32; csrc/rpn.hip writes the arithmetic out):
  1. per (image, level) the min(H * W * A, pre_nms_topk) largest logits over f = (y * W + x) * A + a, descending, in torch.topk's order
     (a NaN above +inf, -0.0 equal to +0.0); among equal values the lower f first (torch leaves this open; it is fixed here);
  2. the anchor of (x, y, a) as grid_anchors gives it, then Box2BoxTransform.apply_deltas (the clamp log(1000 / 16) rounded to float32);
  3. a candidate with a non-finite coordinate or logit is dropped and counted; clip to (h, w); a box is dropped unless
     x2 - x1 > min_box_size and y2 - y1 > min_box_size;
  4. greedy NMS per level within an image: a candidate goes iff a kept one of its level, earlier in the level's order, has
     inter / ((area_a + area_b) - inter) > nms_thresh (detector_inference's formula, 0 / 0 suppresses nothing).  This is torchvision's
     per-class form on the coordinates as they are; Detectron2's batched_nms reaches the coordinate-trick form for small inputs, whose
     shifted boxes can differ in the last bit of an IoU;
  5. an image's survivors by logit descending, then level ascending, then rank within the level; the first post_nms_topk.

Limits (ValueError before any launch): at most 8 levels, A <= 16, pre_nms_topk <= 4096, H * W * A < 2^31 per level.

Out of scope, on purpose:
  * the RPN head's convolutions;
  * anchor labelling / sampling and the RPN losses: they are unmore_amd.rpn_loss (subsample_labels' draw is a stateless hash key per
    anchor there, or keys the caller supplies);
  * anchors that are not a regular grid, and rotated boxes;
  * graph-capture tests, as in the sibling modules.

No CPU fallback."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from . import _tables as T
from .ops import _p, _stream

MAX_LEVELS = 8
MAX_ANCHORS = 16             # per position (csrc/rpn.hip: RPN_MAX_A)
MAX_PRE_NMS_TOPK = 4096      # RPN_MAX_K
SELECT_SHARE = 16384         # scores per workgroup of the partial select (RPN_SELECT_SHARE): a larger level is selected in two steps
COUNTERS = ("candidates", "non_finite", "empty", "suppressed", "kept")
DIVERGED = "Predicted boxes or scores contain Inf/NaN. Training has diverged."


def _int(v, name, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"rpn: {name} must be an integer {'>= ' + str(lo) if hi is None else 'in [' + str(lo) + ', ' + str(hi) + ']'}, "
                         f"got {v!r}")
    return int(v)


def _number(v, name):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"rpn: {name} must be a number, got {v!r}") from None
    if math.isnan(v):
        raise ValueError(f"rpn: {name} is NaN")
    return v


def cell_anchors(sizes, aspect_ratios):
    """DefaultAnchorGenerator.generate_cell_anchors per level: a list of float32 [A, 4] CPU tensors.

    sizes: one sequence of sizes per level; aspect_ratios: one sequence per level, or one sequence broadcast over the levels (as the
    config does).  For each size, then each ratio: w = sqrt(size^2 / ratio), h = ratio * w, the box (-w/2, -h/2, w/2, h/2), computed
    in Python floats and rounded once to float32."""
    try:
        sizes = [[float(s) for s in level] for level in sizes]
        ratios = list(aspect_ratios)
        if ratios and not isinstance(ratios[0], (list, tuple)):
            ratios = [ratios] * len(sizes)
        ratios = [[float(r) for r in level] for level in ratios]
    except (TypeError, ValueError):
        raise ValueError("rpn: sizes is a sequence of sequences of numbers, aspect_ratios one sequence or one per level") from None
    if len(ratios) == 1 and len(sizes) > 1:
        ratios = ratios * len(sizes)
    if not sizes or len(sizes) != len(ratios):
        raise ValueError(f"rpn: {len(sizes)} levels of sizes and {len(ratios)} of aspect ratios")
    out = []
    for k, (ss, rs) in enumerate(zip(sizes, ratios)):
        if not ss or not rs or not all(math.isfinite(v) and v > 0 for v in ss + rs):
            raise ValueError(f"rpn: level {k}: sizes and aspect ratios must be positive and finite, got {ss}, {rs}")
        rows = []
        for s in ss:
            area = s ** 2.0
            for r in rs:
                w = math.sqrt(area / r)
                h = r * w
                rows.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
        out.append(torch.tensor(rows, dtype=torch.float64).to(torch.float32))
    return out


def _check_cells(cells):
    cells = list(cells) if isinstance(cells, (list, tuple)) else [cells]
    if not 1 <= len(cells) <= MAX_LEVELS:
        raise ValueError(f"rpn: between 1 and {MAX_LEVELS} levels, got {len(cells)}")
    for k, c in enumerate(cells):
        if not isinstance(c, torch.Tensor) or c.dtype != torch.float32 or c.dim() != 2 or c.shape[1] != 4 or \
                not 1 <= c.shape[0] <= MAX_ANCHORS:
            raise ValueError(f"rpn: cells[{k}] must be float32 [A, 4] with 1 <= A <= {MAX_ANCHORS}, got {getattr(c, 'dtype', type(c))} "
                             f"{list(getattr(c, 'shape', []))}")
        if c.shape[0] != cells[0].shape[0]:
            raise ValueError(f"rpn: cells[{k}] has {int(c.shape[0])} anchors, cells[0] has {int(cells[0].shape[0])}: the same A on every level")
    return cells


def _check_strides(strides, n_levels, offset):
    strides = list(strides)
    if len(strides) != n_levels:
        raise ValueError(f"rpn: {len(strides)} strides for {n_levels} levels")
    strides = [_int(s, f"strides[{k}]", 1, 1 << 24) for k, s in enumerate(strides)]
    off = _number(offset, "offset")
    if not 0.0 <= off < 1.0:
        raise ValueError(f"rpn: offset must lie in [0, 1), got {offset!r}")
    for s in strides:
        if float(np.float32(off * s)) != off * s:
            raise ValueError(f"rpn: offset * stride = {off!r} * {s} is not exactly representable in float32")
    return strides, off


def grid_anchors(cells, strides, feature_sizes, offset=0.0):
    """DefaultAnchorGenerator's anchors of whole level maps: a list of float32 [H * W * A, 4] tensors on the cells' device, in (y, x, a)
    order.  Anchor (y, x, a) = (sx, sy, sx, sy) + cells[l][a] with sx = x * stride + offset * stride and sy likewise in y, one float32
    add per coordinate.  strides: positive integers; offset in [0, 1) with offset * stride exactly representable in float32."""
    cells = _check_cells(cells)
    strides, off = _check_strides(strides, len(cells), offset)
    sizes = list(feature_sizes)
    if len(sizes) != len(cells):
        raise ValueError(f"rpn: {len(sizes)} feature sizes for {len(cells)} levels")
    out = []
    for k, (c, s, hw) in enumerate(zip(cells, strides, sizes)):
        try:
            h, w = hw
        except (TypeError, ValueError):
            raise ValueError(f"rpn: feature_sizes[{k}] must be (H, W), got {hw!r}") from None
        h, w = _int(h, f"feature_sizes[{k}][0]", 1), _int(w, f"feature_sizes[{k}][1]", 1)
        if h * s > 1 << 24 or w * s > 1 << 24:
            raise ValueError(f"rpn: level {k}: H * stride and W * stride must be at most 2^24")
        o = torch.tensor(off * s, dtype=torch.float32, device=c.device)
        sx = torch.arange(w, dtype=torch.int64, device=c.device).mul(s).to(torch.float32) + o
        sy = torch.arange(h, dtype=torch.int64, device=c.device).mul(s).to(torch.float32) + o
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        shifts = torch.stack((xx, yy, xx, yy), dim=2).reshape(-1, 1, 4)
        out.append((shifts + c.reshape(1, -1, 4)).reshape(-1, 4))
    return out


def _check_args(logits, deltas, cells, strides, image_sizes, nms_thresh, pre_nms_topk, post_nms_topk, min_box_size, box2box_weights, offset):
    """every check that needs no device: (logits, deltas, cells, strides, sizes, N, A, thresholds ...)"""
    if not isinstance(logits, (list, tuple)) or not isinstance(deltas, (list, tuple)) or not logits or len(logits) != len(deltas):
        raise ValueError("rpn: pred_objectness_logits and pred_anchor_deltas are lists with one tensor per level, of the same length")
    cells = _check_cells(cells)
    if len(cells) != len(logits):
        raise ValueError(f"rpn: {len(cells)} levels of cell anchors for {len(logits)} levels of logits")
    strides, off = _check_strides(strides, len(cells), offset)
    A = int(cells[0].shape[0])
    N = None
    for k, (s, d) in enumerate(zip(logits, deltas)):
        for t, name in ((s, "pred_objectness_logits"), (d, "pred_anchor_deltas")):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype not in (torch.float32, torch.bfloat16) or min(t.shape) < 1:
                raise ValueError(f"rpn: {name}[{k}] must be float32 or bfloat16 [N, C, H, W] with no empty dimension, got "
                                 f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")
            if t.dtype != logits[0].dtype:
                raise ValueError(f"rpn: {name}[{k}] is {t.dtype}, pred_objectness_logits[0] is {logits[0].dtype}: one type for all")
            if not t.is_contiguous():
                raise ValueError(f"rpn: {name}[{k}] is not contiguous: the head's outputs are read in place")
        if N is None:
            N = int(s.shape[0])
        if s.shape[0] != N or s.shape[1] != A or tuple(d.shape) != (N, 4 * A, s.shape[2], s.shape[3]):
            raise ValueError(f"rpn: level {k}: logits {list(s.shape)} and deltas {list(d.shape)}; expected [{N}, {A}, H, W] and "
                             f"[{N}, {4 * A}, H, W]")
        h, w = int(s.shape[2]), int(s.shape[3])
        if h * w * A >= 1 << 31:
            raise ValueError(f"rpn: level {k}: H * W * A = {h * w * A}, 2^31 or more")
        if h * strides[k] > 1 << 24 or w * strides[k] > 1 << 24:
            raise ValueError(f"rpn: level {k}: H * stride and W * stride must be at most 2^24")
    sizes = []
    shapes = list(image_sizes)
    if len(shapes) != N:
        raise ValueError(f"rpn: {len(shapes)} image sizes for {N} images")
    for k, s in enumerate(shapes):
        try:
            h, w = (float(v) for v in s)
        except (TypeError, ValueError):
            raise ValueError(f"rpn: image_sizes[{k}] must be (h, w), got {s!r}") from None
        if not (math.isfinite(h) and math.isfinite(w) and h >= 0 and w >= 0):
            raise ValueError(f"rpn: image_sizes[{k}] must be finite and non-negative, got {s!r}")
        sizes.append((h, w))
    nt, mb = _number(nms_thresh, "nms_thresh"), _number(min_box_size, "min_box_size")
    pre = _int(pre_nms_topk, "pre_nms_topk", 1, MAX_PRE_NMS_TOPK)
    post = _int(post_nms_topk, "post_nms_topk", 1)
    try:
        bw = tuple(float(v) for v in box2box_weights)
    except (TypeError, ValueError):
        raise ValueError(f"rpn: box2box_weights must be four numbers, got {box2box_weights!r}") from None
    if len(bw) != 4 or not all(math.isfinite(v) and v > 0 for v in bw):
        raise ValueError(f"rpn: box2box_weights must be four positive finite numbers, got {box2box_weights!r}")
    if N * len(cells) > 65535:
        raise ValueError(f"rpn: {N} images x {len(cells)} levels: at most 65535 (image, level) pairs per call")
    return list(logits), list(deltas), cells, strides, off, sizes, N, A, nt, pre, post, mb, bw


def rpn_proposals(pred_objectness_logits, pred_anchor_deltas, cells, strides, image_sizes, *, nms_thresh, pre_nms_topk, post_nms_topk,
                  min_box_size=0.0, training=False, box2box_weights=(1.0, 1.0, 1.0, 1.0), offset=0.0, padded=False, stats=None,
                  _debug=None, _phase_ms=None):
    """Detectron2's RPN.predict_proposals for the whole batch: the module docstring lists the steps.

    pred_objectness_logits[l]: [N, A, H_l, W_l]; pred_anchor_deltas[l]: [N, 4A, H_l, W_l] with channel a * 4 + c -- the head's raw
    outputs, float32 or bfloat16 (widened), contiguous, read in place.  cells: cell_anchors' result; strides: the levels' strides;
    image_sizes: (h, w) per image.  pre_nms_topk / post_nms_topk: the recipe's 2000 / 4000 in training and 1000 / 1000 at inference.

    Returns a list of (proposal_boxes float32 [n, 4], objectness_logits float32 [n]) per image, views of one padded buffer, after ONE
    host read of the per-image counts and non-finite counts.  training=True with a non-finite candidate raises FloatingPointError, as
    Detectron2 does; at inference such candidates are dropped.  padded=True returns (boxes [N, cap, 4], logits [N, cap], counts int32
    [N]) on the device, zero past the count, with NO host read (and so no FloatingPointError), cap = min(post_nms_topk, sum over the
    levels of min(H * W * A, pre_nms_topk)).

    stats: a dict that receives `counters`, int32 [N, L, 5] ON THE DEVICE in the order of COUNTERS: candidates, dropped as non-finite,
    dropped as empty, suppressed by the NMS, kept by the NMS (before the truncation to post_nms_topk); and `scalars`, a function that
    reads them and gives their sums by name.
    ValueError for argument errors before any launch, RuntimeError off the GPU.  No float atomics: the same input gives the same bytes."""
    logits, deltas, cells, strides, off, sizes, N, A, nt, pre, post, mb, bw = _check_args(
        pred_objectness_logits, pred_anchor_deltas, cells, strides, image_sizes, nms_thresh, pre_nms_topk, post_nms_topk, min_box_size,
        box2box_weights, offset)
    dev = T.one_device(logits + deltas, "rpn", "rpn_proposals")
    nl = len(logits)
    ks = [min(int(s.shape[2] * s.shape[3]) * A, pre) for s in logits]
    total = sum(ks)
    cap = min(post, total)
    if N * total >= 1 << 31:
        raise ValueError(f"rpn: {N} images x {total} candidates: 2^31 or more")
    tab = (ctypes.c_int64 * (5 * nl))()
    for k, (s, d) in enumerate(zip(logits, deltas)):
        tab[5 * k:5 * k + 5] = [s.data_ptr(), d.data_ptr(), int(s.shape[2]), int(s.shape[3]), strides[k]]
    host = np.zeros(nl * MAX_ANCHORS * 4 + N * 2, dtype=np.float32)
    for k, c in enumerate(cells):
        host[k * MAX_ANCHORS * 4:k * MAX_ANCHORS * 4 + A * 4] = c.detach().cpu().numpy().reshape(-1)
    host[nl * MAX_ANCHORS * 4:] = np.asarray(sizes, dtype=np.float32).reshape(-1)
    with torch.cuda.device(dev):
        params = torch.from_numpy(host).to(dev)
        cells_d, sizes_d = params[:nl * MAX_ANCHORS * 4], params[nl * MAX_ANCHORS * 4:]
        boxes = torch.zeros((N, cap, 4), dtype=torch.float32, device=dev)
        scores = torch.zeros((N, cap), dtype=torch.float32, device=dev)
        counts = torch.empty(N, dtype=torch.int32, device=dev)
        counters = torch.empty((N, nl, 5), dtype=torch.int32, device=dev)
        c_box = torch.empty((N, total, 4), dtype=torch.float32, device=dev)
        c_score = torch.empty((N, total), dtype=torch.float32, device=dev)
        c_idx = torch.empty((N, total), dtype=torch.int32, device=dev)
        c_flag = torch.empty((N, total), dtype=torch.uint8, device=dev)
        c_raw = torch.empty((N, total, 4), dtype=torch.float32, device=dev) if _debug is not None else None
        nbytes = L.lib().umr_rpn_workspace(tab, nl, N, A, pre)
        ws = T.workspace(nbytes, dev)

        def launch(phases):
            L.check(L.lib().umr_rpn_proposals(tab, nl, N, A, T.dtype_code(logits[0]), _p(cells_d), _p(sizes_d), pre, post, nt, mb, bw[0],
                                              bw[1], bw[2], bw[3], off, phases, _p(c_box), _p(c_score), _p(c_idx), _p(c_flag), _p(c_raw),
                                              _p(boxes), _p(scores), _p(counts), _p(counters), _p(ws), nbytes, _stream()),
                    "umr_rpn_proposals")
        parts = (("select", 2), ("suppression", 4), ("scan", 8), ("merge", 16))
        if any(int(s.shape[2] * s.shape[3]) * A > SELECT_SHARE for s in logits):
            parts = (("partial_select", 1),) + parts
        T.timed(launch, parts, _phase_ms)
    if stats is not None:
        def scalars():
            """the counters summed over images and levels, read from the device when asked"""
            return dict(zip(COUNTERS, counters.sum(dim=(0, 1)).tolist()))
        stats["counters"], stats["scalars"] = counters, scalars
    if _debug is not None:
        first = [0]
        for k in ks:
            first.append(first[-1] + k)
        _debug.update(boxes=c_box, scores=c_score, indices=c_idx, flags=c_flag, raw_boxes=c_raw, level_first=first)
    if padded:
        return boxes, scores, counts
    got = torch.cat((counts, counters[:, :, 1].sum(dim=1, dtype=torch.int32))).tolist()      # the one host read
    if training and any(got[N:]):
        raise FloatingPointError(DIVERGED)
    return [(boxes[k, :got[k]], scores[k, :got[k]]) for k in range(N)]
