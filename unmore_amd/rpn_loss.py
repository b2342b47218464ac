"""The training half of the stage-3 detector's RPN on the device: Detectron2's RPN.label_and_sample_anchors and RPN.losses, the two
calls that RPN.forward makes in training besides the proposal step of unmore_amd.rpn (cad/modeling/meta_arch/rcnn.py:165, 333:
self.proposal_generator(images, features, gt_instances)).

  label_and_sample_anchors   per image: IoU of every anchor with the image's ground truths, the matcher's labels, the low-quality matches,
                             the boundary filter and the sample of batch_size_per_image anchors: three launches for the whole batch,
                             four when an image has more than SELECT_SHARE anchors
  rpn_losses                 loss_rpn_cls and loss_rpn_loc over the sampled anchors with their gradients: two launches

The anchors are rpn.grid_anchors' (level after level, inside a level f = (y * W + x) * A + a, r the global index, R per image); the
kernels rebuild them from (x, y, a) and never read an anchor tensor, no [G, R] matrix is stored, and neither call reads the device back.
The semantics (tests/rpn_loss_common.py restates them in NumPy; csrc/rpn_loss.hip writes the arithmetic out):
  1. IoU = box_loss's pairwise_iou (0 unless inter > 0, correctly rounded division: the float32 NumPy value bit for bit).  Per anchor
     the maximum over the image's ground truths and the FIRST index that reaches it (torch.max(dim=0) in CPU order).  With thresholds
     (lo, hi) rounded to float32: label 0 if v < lo, -1 if lo <= v < hi, 1 if v >= hi.  An image without ground truths: all labels 0,
     matched index 0.
  2. allow_low_quality_matches: anchor r becomes 1 if for some ground truth g IoU(g, r) equals the maximum of row g over all anchors,
     exactly.  The matched index is NOT changed (Detectron2's behaviour).  Its quirk stays: a finite ground truth that overlaps no anchor
     has row maximum 0 and marks every anchor of IoU 0 with it, which is every anchor.  Departure: a ground truth with a non-finite
     coordinate takes no part in steps 1 and 2 and is counted in the `bad` counter (the kernels cannot raise; Detectron2 would hand the
     NaN on).
  3. anchor_boundary_thresh t >= 0: label -1 unless x1 >= -t, y1 >= -t, x2 < w + t and y2 < h + t.  Negative (the default): off.
  4. With B = batch_size_per_image, P and Q the numbers of labels 1 and 0: num_pos = min(P, int(B * positive_fraction)), num_neg =
     min(Q, B - num_pos).  The num_pos positives with the LARGEST key are taken, equal keys to the lower r; likewise the negatives; every
     other anchor becomes -1.  Keys are 31-bit non-negative integers: `keys`, int32 [N, R], with which a caller imposes any order (one
     drawn on the host included; only the low 31 bits count); or, by default, a stateless hash of (seed, image, r) computed in the kernel:
         fmix(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16     (mod 2^32; murmur3's finaliser)
         key = fmix(fmix(r ^ (seed & 0xffffffff)) ^ ((n * 0x9e3779b9 + (seed >> 32)) mod 2^32)) >> 1
     `seed` is a Python int the caller passes per step (taken mod 2^64).  This is a uniform sample without replacement like
     subsample_labels' randperm(P)[:k]; it is not the same draw, consumes no device RNG state and reads nothing back.
  5. Over the sampled anchors binary_cross_entropy_with_logits(logit, label, "sum"); over the sampled positives smooth-L1 (beta 0: L1,
     gradient sign(p - t), 0 at 0) of the deltas against Box2BoxTransform.get_deltas(anchor, matched ground truth); both divided by
     B * N and multiplied by their loss_weight.  Logits and deltas float32 or bfloat16, widened; the terms are formed in float64.

Limits (ValueError before any launch): those of rpn.py (8 levels, A <= 16, R < 2^31) and batch_size_per_image <= 1024.
Out of scope: the IoU box-regression losses (the recipe uses smooth_l1), rotated boxes, graph-capture tests.  No CPU fallback."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from . import _tables as T
from .ops import _p, _stream
from .rpn import MAX_ANCHORS, _check_cells, _check_strides, _int, _number

MAX_BATCH = 1024             # csrc/rpn_loss.hip: RL_MAX_BATCH
SELECT_SHARE = 16384         # anchors per workgroup of the partial select (RL_SELECT_SHARE): more anchors per image are sampled in two steps
COUNTERS = ("positives", "negatives", "sampled_positives", "sampled_negatives", "bad")


class AnchorSamples:
    """label_and_sample_anchors' result: index, gt int32 [N, B] and counts int32 [N, 2] on the device (first the counts[n, 0] positives in
    ascending r, then the counts[n, 1] negatives in ascending r; entries past the counts are not defined); with dense=True also labels
    int8 [N, R] after sampling and matched_idxs int32 [N, R]."""
    __slots__ = ("index", "gt", "counts", "labels", "matched_idxs", "num_anchors", "batch_size_per_image")

    def __init__(self, index, gt, counts, labels, matched_idxs, num_anchors, batch_size_per_image):
        self.index, self.gt, self.counts, self.labels, self.matched_idxs = index, gt, counts, labels, matched_idxs
        self.num_anchors, self.batch_size_per_image = num_anchors, batch_size_per_image


def _geometry(cells, strides, feature_sizes, offset):
    """(cells, strides, offset, [(H, W)], A, R) of the checked anchor grid"""
    cells = _check_cells(cells)
    strides, off = _check_strides(strides, len(cells), offset)
    sizes = list(feature_sizes)
    if len(sizes) != len(cells):
        raise ValueError(f"rpn_loss: {len(sizes)} feature sizes for {len(cells)} levels")
    A, maps, R = int(cells[0].shape[0]), [], 0
    for k, (s, hw) in enumerate(zip(strides, sizes)):
        try:
            h, w = hw
        except (TypeError, ValueError):
            raise ValueError(f"rpn_loss: feature_sizes[{k}] must be (H, W), got {hw!r}") from None
        h, w = _int(h, f"feature_sizes[{k}][0]", 1), _int(w, f"feature_sizes[{k}][1]", 1)
        if h * s > 1 << 24 or w * s > 1 << 24:
            raise ValueError(f"rpn_loss: level {k}: H * stride and W * stride must be at most 2^24")
        maps.append((h, w))
        R += h * w * A
    if R >= (1 << 31) - 1:
        raise ValueError(f"rpn_loss: {R} anchors per image, 2^31 - 1 or more")
    return cells, strides, off, maps, A, R


def _ground_truths(gt_boxes, N):
    """the list of [G_i, 4] float32 tensors (or objects with .tensor) -> (tensors, prefix table as a Python list)"""
    if not isinstance(gt_boxes, (list, tuple)) or len(gt_boxes) != N:
        raise ValueError(f"rpn_loss: gt_boxes is a list with one [G, 4] tensor per image, {N} of them")
    out, first = [], [0]
    for k, g in enumerate(gt_boxes):
        g = T.unwrap(g)
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.dim() != 2 or g.shape[1] != 4:
            raise ValueError(f"rpn_loss: gt_boxes[{k}] must be float32 [G, 4], got {getattr(g, 'dtype', type(g))} "
                             f"{list(getattr(g, 'shape', []))}")
        out.append(g)
        first.append(first[-1] + int(g.shape[0]))
    if first[-1] >= (1 << 31) - 1:
        raise ValueError("rpn_loss: 2^31 - 1 ground truths or more")
    return out, first


def _upload(cells, A, extra_f32, first, dev):
    """one host-to-device copy: the cell anchors [L, 16, 4] float32, `extra_f32`, the int32 prefix table -> their device views"""
    nl = len(cells)
    host = np.zeros(nl * MAX_ANCHORS * 4 + len(extra_f32) + len(first), dtype=np.float32)
    for k, c in enumerate(cells):
        host[k * MAX_ANCHORS * 4:k * MAX_ANCHORS * 4 + A * 4] = c.detach().cpu().numpy().reshape(-1)
    a, b = nl * MAX_ANCHORS * 4, nl * MAX_ANCHORS * 4 + len(extra_f32)
    host[a:b] = extra_f32
    host[b:] = np.asarray(first, dtype=np.int32).view(np.float32)
    params = torch.from_numpy(host).to(dev)
    return params[:a], params[a:b], params[b:].view(torch.int32)


def _cat_gt(gts, dev):
    return torch.cat(gts).contiguous() if gts else torch.zeros((0, 4), dtype=torch.float32, device=dev)


def label_and_sample_anchors(cells, strides, feature_sizes, gt_boxes, image_sizes, *, iou_thresholds=(0.3, 0.7), iou_labels=(0, -1, 1),
                             allow_low_quality_matches=True, batch_size_per_image=256, positive_fraction=0.5, anchor_boundary_thresh=-1,
                             offset=0.0, seed=0, keys=None, dense=False, stats=None, _debug=None, _phase_ms=None):
    """Detectron2's RPN.label_and_sample_anchors for the whole batch: the module docstring lists the steps.

    cells: rpn.cell_anchors' result; strides: the levels' strides; feature_sizes: (H, W) per level; gt_boxes: a list of float32 [G_i, 4]
    device tensors or objects with .tensor (one torch.cat and an int32 [N + 1] prefix table are the upload); image_sizes: (h, w) per
    image.  seed: a Python int per step; keys: int32 [N, R] on the device instead of the hash (non-negative; the low 31 bits count).

    Returns AnchorSamples.  stats: a dict that receives `counters`, int32 [N, 5] ON THE DEVICE in the order of COUNTERS (P, Q, sampled
    positives, sampled negatives, bad ground truths), and `scalars`, a function that reads them when asked and gives Detectron2's logged
    rpn/num_pos_anchors and rpn/num_neg_anchors (the sampled counts averaged over the images) and `bad`.  _debug: a dict that receives
    matched_vals float32 [N, R], matched_idxs int32 [N, R], labels int8 [N, R] BEFORE sampling and row_max float32 [sum of G].
    ValueError for argument errors before any launch, RuntimeError off the GPU.  The same input gives the same bytes."""
    cells, strides, off, maps, A, R = _geometry(cells, strides, feature_sizes, offset)
    shapes = list(image_sizes)
    N = len(shapes)
    if not 1 <= N <= 65535:
        raise ValueError(f"rpn_loss: between 1 and 65535 images, got {N}")
    sizes = []
    for k, s in enumerate(shapes):
        try:
            h, w = (float(v) for v in s)
        except (TypeError, ValueError):
            raise ValueError(f"rpn_loss: image_sizes[{k}] must be (h, w), got {s!r}") from None
        if not (math.isfinite(h) and math.isfinite(w) and h >= 0 and w >= 0):
            raise ValueError(f"rpn_loss: image_sizes[{k}] must be finite and non-negative, got {s!r}")
        sizes += [h, w]
    gts, first = _ground_truths(gt_boxes, N)
    try:
        th, labels3 = [float(v) for v in iou_thresholds], [int(v) for v in iou_labels]
    except (TypeError, ValueError):
        raise ValueError(f"rpn_loss: iou_thresholds {iou_thresholds!r} and iou_labels {iou_labels!r} must be numbers") from None
    if len(th) != 2 or labels3 != [0, -1, 1]:
        raise ValueError(f"rpn_loss: two iou_thresholds with iou_labels (0, -1, 1) are supported, got {iou_thresholds!r} and {iou_labels!r}")
    if not all(math.isfinite(v) for v in th) or th[0] > th[1]:
        raise ValueError(f"rpn_loss: iou_thresholds must be finite and ordered, got {iou_thresholds!r}")
    B = _int(batch_size_per_image, "batch_size_per_image", 1, MAX_BATCH)
    frac = _number(positive_fraction, "positive_fraction")
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"rpn_loss: positive_fraction must lie in [0, 1], got {positive_fraction!r}")
    pos_cap = int(B * frac)
    bt = _number(anchor_boundary_thresh, "anchor_boundary_thresh")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"rpn_loss: seed must be an integer, got {seed!r}")
    seed = int(seed) & ((1 << 64) - 1)
    tensors = gts + ([keys] if keys is not None else [])
    if keys is not None and (not isinstance(keys, torch.Tensor) or keys.dtype != torch.int32 or tuple(keys.shape) != (N, R) or
                             not keys.is_contiguous()):
        raise ValueError(f"rpn_loss: keys must be a contiguous int32 [{N}, {R}] tensor, got {getattr(keys, 'dtype', type(keys))} "
                         f"{list(getattr(keys, 'shape', []))}")
    dev = T.one_device(tensors, "rpn_loss", "label_and_sample_anchors")
    nl = len(cells)
    tab = (ctypes.c_int64 * (3 * nl))()
    for k, ((h, w), s) in enumerate(zip(maps, strides)):
        tab[3 * k:3 * k + 3] = [h, w, s]
    with torch.cuda.device(dev):
        cells_d, sizes_d, first_d = _upload(cells, A, sizes, first, dev)
        gt = _cat_gt(gts, dev)
        mval = torch.empty((N, R), dtype=torch.float32, device=dev)
        midx = torch.empty((N, R), dtype=torch.int32, device=dev)
        row_max = torch.empty(max(first[-1], 1), dtype=torch.float32, device=dev)
        labels = torch.empty((N, R), dtype=torch.int8, device=dev)
        index = torch.empty((N, B), dtype=torch.int32, device=dev)
        sgt = torch.empty((N, B), dtype=torch.int32, device=dev)
        counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
        counters = torch.empty((N, 5), dtype=torch.int32, device=dev)
        dense_labels = torch.empty((N, R), dtype=torch.int8, device=dev) if dense else None
        nbytes = L.lib().umr_rpn_label_workspace(tab, nl, N, A, B)
        ws = T.workspace(nbytes, dev)

        def launch(phases):
            L.check(L.lib().umr_rpn_label_sample(tab, nl, N, A, _p(cells_d), _p(sizes_d), _p(gt) if first[-1] else None, _p(first_d),
                                                 first[-1], th[0], th[1], 1 if allow_low_quality_matches else 0, B, pos_cap, bt, off,
                                                 ctypes.c_int64(seed).value, _p(keys) if keys is not None else None, phases, _p(mval),
                                                 _p(midx), _p(row_max), _p(labels), _p(index), _p(sgt), _p(counts),
                                                 _p(dense_labels) if dense else None, _p(counters), _p(ws), nbytes, _stream()),
                    "umr_rpn_label_sample")
        parts = (("match", 1), ("label", 2), ("select", 8))
        if R > SELECT_SHARE:
            parts = parts[:2] + (("partial_select", 4),) + parts[2:]
        T.timed(launch, parts, _phase_ms)
    if stats is not None:
        def scalars():
            """Detectron2's logged counts, read from the device when asked"""
            c = counters.sum(dim=0).tolist()
            return {"rpn/num_pos_anchors": c[2] / N, "rpn/num_neg_anchors": c[3] / N, "bad": int(c[4])}
        stats["counters"], stats["scalars"] = counters, scalars
    if _debug is not None:
        _debug.update(matched_vals=mval, matched_idxs=midx, labels=labels, row_max=row_max[:first[-1]], gt_first=first)
    return AnchorSamples(index, sgt, counts, dense_labels, midx if dense else None, R, B)


class _RpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, run, n_levels, *maps):
        loss_cls, loss_loc, grads = run([m.detach() for m in maps])
        ctx.save_for_backward(*grads)
        ctx.n_levels = n_levels
        return loss_cls, loss_loc

    @staticmethod
    def backward(ctx, g_cls, g_loc):
        nl = ctx.n_levels                                  # the saved maps times their own incoming scalar, in the inputs' type
        g = ctx.saved_tensors
        return (None, None) + tuple(m * g_cls for m in g[:nl]) + tuple(m * g_loc for m in g[nl:])


def _loss_weights(loss_weight):
    if isinstance(loss_weight, dict):
        unknown = set(loss_weight) - {"loss_rpn_cls", "loss_rpn_loc"}
        if unknown:
            raise ValueError(f"rpn_loss: loss_weight has the keys loss_rpn_cls / loss_rpn_loc, got {sorted(unknown)}")
        w = (loss_weight.get("loss_rpn_cls", 1.0), loss_weight.get("loss_rpn_loc", 1.0))
    else:
        w = (loss_weight, loss_weight)
    w = tuple(_number(v, "loss_weight") for v in w)
    if not all(math.isfinite(v) for v in w):
        raise ValueError(f"rpn_loss: loss_weight must be finite, got {loss_weight!r}")
    return w


def rpn_losses(pred_objectness_logits, pred_anchor_deltas, samples, cells, strides, gt_boxes, *, box2box_weights=(1.0, 1.0, 1.0, 1.0),
               smooth_l1_beta=0.0, box_reg_loss_type="smooth_l1", batch_size_per_image=256, loss_weight=1.0, offset=0.0, stats=None,
               _phase_ms=None):
    """Detectron2's RPN.losses on label_and_sample_anchors' samples: {"loss_rpn_cls", "loss_rpn_loc"}, float32 scalars on the device.

    pred_objectness_logits[l]: [N, A, H_l, W_l]; pred_anchor_deltas[l]: [N, 4A, H_l, W_l] with channel a * 4 + c -- the head's raw
    outputs, float32 or bfloat16, contiguous, read in place.  gt_boxes: as given to label_and_sample_anchors.  batch_size_per_image is the
    normaliser B of 1 / (B * N) and must be the samples'.  loss_weight: a number for both losses or a dict with loss_rpn_cls /
    loss_rpn_loc (a missing key: 1).

    Both losses are differentiable with respect to every level's logits and deltas through one autograd.Function: the forward launch also
    writes d loss_rpn_cls / d logits = (sigmoid(x) - label) w / (B N) and d loss_rpn_loc / d deltas into maps that are zero outside the
    samples, in the inputs' type and layout, and backward multiplies each by its incoming scalar.  stats: receives `samples` (the counts
    tensor).  ValueError for argument errors before any launch, RuntimeError off the GPU; nothing is read back."""
    if box_reg_loss_type != "smooth_l1":
        raise ValueError(f"rpn_loss: box_reg_loss_type {box_reg_loss_type!r} is not supported: only 'smooth_l1' (the recipe's) is")
    if not isinstance(samples, AnchorSamples):
        raise ValueError("rpn_loss: samples is label_and_sample_anchors' result")
    if not isinstance(pred_objectness_logits, (list, tuple)) or not isinstance(pred_anchor_deltas, (list, tuple)) or \
            not pred_objectness_logits or len(pred_objectness_logits) != len(pred_anchor_deltas):
        raise ValueError("rpn_loss: pred_objectness_logits and pred_anchor_deltas are lists with one tensor per level, of the same length")
    logits, deltas = list(pred_objectness_logits), list(pred_anchor_deltas)
    for k, (s, d) in enumerate(zip(logits, deltas)):
        for t, name in ((s, "pred_objectness_logits"), (d, "pred_anchor_deltas")):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype not in (torch.float32, torch.bfloat16) or min(t.shape) < 1:
                raise ValueError(f"rpn_loss: {name}[{k}] must be float32 or bfloat16 [N, C, H, W] with no empty dimension, got "
                                 f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")
            if t.dtype != logits[0].dtype:
                raise ValueError(f"rpn_loss: {name}[{k}] is {t.dtype}, pred_objectness_logits[0] is {logits[0].dtype}: one type for all")
            if not t.is_contiguous():
                raise ValueError(f"rpn_loss: {name}[{k}] is not contiguous: the head's outputs are read in place")
    cells, strides, off, maps, A, R = _geometry(cells, strides, [tuple(s.shape[2:]) for s in logits], offset)
    N = int(logits[0].shape[0])
    for k, (s, d) in enumerate(zip(logits, deltas)):
        if tuple(s.shape[:2]) != (N, A) or tuple(d.shape) != (N, 4 * A, s.shape[2], s.shape[3]):
            raise ValueError(f"rpn_loss: level {k}: logits {list(s.shape)} and deltas {list(d.shape)}; expected [{N}, {A}, H, W] and "
                             f"[{N}, {4 * A}, H, W]")
    B = _int(batch_size_per_image, "batch_size_per_image", 1, MAX_BATCH)
    if samples.num_anchors != R or samples.batch_size_per_image != B or tuple(samples.index.shape) != (N, B):
        raise ValueError(f"rpn_loss: the samples are of {samples.num_anchors} anchors, batch {samples.batch_size_per_image}, "
                         f"{int(samples.index.shape[0])} images; the predictions of {R} anchors, batch {B}, {N} images")
    gts, first = _ground_truths(gt_boxes, N)
    try:
        bw = tuple(float(v) for v in box2box_weights)
    except (TypeError, ValueError):
        raise ValueError(f"rpn_loss: box2box_weights must be four numbers, got {box2box_weights!r}") from None
    if len(bw) != 4 or not all(math.isfinite(v) and v > 0 for v in bw):
        raise ValueError(f"rpn_loss: box2box_weights must be four positive finite numbers, got {box2box_weights!r}")
    beta = _number(smooth_l1_beta, "smooth_l1_beta")
    if not (beta >= 0 and math.isfinite(beta)):
        raise ValueError(f"rpn_loss: smooth_l1_beta must be >= 0 and finite, got {smooth_l1_beta!r}")
    w_cls, w_loc = _loss_weights(loss_weight)
    dev = T.one_device(logits + deltas + gts + [samples.index, samples.gt, samples.counts], "rpn_loss", "rpn_losses")
    nl = len(logits)
    dtype = logits[0].dtype

    def run(maps_in):
        lg, dl = maps_in[:nl], maps_in[nl:]
        with torch.cuda.device(dev):
            cells_d, _, first_d = _upload(cells, A, [], first, dev)
            gt = _cat_gt(gts, dev)
            # one zeroed buffer for all gradient maps: the launch stores only at the samples
            numels = [t.numel() for t in lg + dl]
            starts = np.concatenate([[0], np.cumsum([(n + 7) // 8 * 8 for n in numels])])
            flat = torch.zeros(int(starts[-1]), dtype=dtype, device=dev)
            grads = [flat[int(a):int(a) + n].view(t.shape) for a, n, t in zip(starts[:-1], numels, lg + dl)]
            tab = (ctypes.c_int64 * (7 * nl))()
            for k in range(nl):
                tab[7 * k:7 * k + 7] = [maps[k][0], maps[k][1], strides[k], lg[k].data_ptr(), dl[k].data_ptr(), grads[k].data_ptr(),
                                        grads[nl + k].data_ptr()]
            out = torch.empty(2, dtype=torch.float32, device=dev)
            nbytes = L.lib().umr_rpn_loss_workspace(N)
            ws = T.workspace(nbytes, dev)

            def launch(phases):
                L.check(L.lib().umr_rpn_loss(tab, nl, N, A, T.dtype_code(lg[0]), _p(cells_d), _p(gt) if first[-1] else None, _p(first_d),
                                             first[-1], _p(samples.index), _p(samples.gt), _p(samples.counts), B, bw[0], bw[1], bw[2], bw[3],
                                             beta, w_cls / (B * N), w_loc / (B * N), off, phases, _p(out), _p(ws), nbytes, _stream()),
                        "umr_rpn_loss")
            T.timed(launch, (("terms", 1), ("sum", 2)), _phase_ms)
        return out[0], out[1], grads

    loss_cls, loss_loc = _RpnLoss.apply(run, nl, *(logits + deltas))
    if stats is not None:
        stats["samples"] = samples.counts
    return {"loss_rpn_cls": loss_cls, "loss_rpn_loc": loss_loc}
