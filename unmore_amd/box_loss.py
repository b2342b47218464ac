"""The box branch of the stage-3 detector's cascade ROI heads on the device (cad/modeling/roi_heads/custom_cascade_rcnn.py:166-357,
CustomCascadeROIHeads under the recipe's NUM_CLASSES 1, CLS_AGNOSTIC_BBOX_REG, USE_SOFT_TARGETS and USE_DROPLOSS; fast_rcnn.py:94-121,
329-390, 462-514, 574-598; cad/structures/boxes.py; cad/modeling/box_regression.py).  Three calls per cascade stage replace the
reference's several dozen small launches and its host reads: `match_and_label` (_match_and_label_boxes), `fast_rcnn_losses`
(the drop-loss block of _forward_box + FastRCNNOutputLayers.losses, with both gradients) and `next_stage_proposals` (predict_boxes +
_create_proposals_from_boxes).  `apply_deltas`, `get_deltas` and `droploss_weights` expose the pieces.  The matcher's index comes
back as `mask_index`, which is what mask_loss.mask_rcnn_loss_weighted reads the masks through.  No CPU fallback:
tests/box_loss_common.py restates the method in NumPy and torch CPU ops (csrc/box_loss.hip writes the arithmetic out)."""
import math

import torch

from . import _lib as L
from . import _tables as T
from .ops import _p, _stream

CHUNK = 256                  # proposals per workgroup (csrc/box_loss.hip: BL_THREADS)
GT_TILE = 256                # ground truths staged in LDS at a time (BL_GT_TILE)
UNIQUE_ROWS = 100            # the reference's gt_boxes.tensor[:100]
SCALE_CLAMP = math.log(1000.0 / 16)
COUNTERS = ("rows", "fg", "accurate", "fg_accurate", "false_negative", "dropped", "bad")


def _check_boxes(b, what, name):
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or b.dim() != 2 or b.shape[1] != 4:
        raise ValueError(f"box_loss: {what}: {name} must be float32 [n, 4], got {getattr(b, 'dtype', type(b))} {list(getattr(b, 'shape', []))}")
    return int(b.shape[0])


def _check_vector(v, n, what, name, integer):
    ok = isinstance(v, torch.Tensor) and tuple(v.shape) == (n,)
    if ok and integer:
        ok = not v.dtype.is_floating_point and not v.dtype.is_complex and v.dtype != torch.bool
    elif ok:
        ok = v.dtype == torch.float32
    if not ok:
        raise ValueError(f"box_loss: {what}: {name} must be {'integer' if integer else 'float32'} [{n}], got {getattr(v, 'dtype', type(v))} "
                         f"{list(getattr(v, 'shape', []))}")


def _device(tensors, what):
    return T.one_device(tensors, "box_loss", what)


def _weights4(w):
    try:
        w = tuple(float(v) for v in w)
    except TypeError:
        w = ()
    if len(w) != 4 or not all(v > 0 and math.isfinite(v) for v in w):
        raise ValueError(f"box_loss: box2box_weights must be four positive numbers (wx, wy, ww, wh), got {w!r}")
    return w


def _chunks(n):
    return (n + CHUNK - 1) // CHUNK


def _upload_table(images, dev):
    """one umr_bl_image per image -- (boxes, gt_boxes, gt_classes, gt_scores, (height, width)), None where the call does not read it --
    in one host-to-device copy: (device buffer, what the table points into, R, number of chunks)"""
    tab = (L.BlImage * max(len(images), 1))()
    hold, first, chunk = [], 0, 0
    for k, (boxes, gtb, gtc, gts, size) in enumerate(images):
        ts = [None if t is None else t.contiguous() for t in (boxes, gtb, gtc, gts)]
        hold += ts
        e = tab[k]
        e.boxes, e.gt_boxes, e.gt_classes, e.gt_scores = (None if t is None or t.numel() == 0 else t.data_ptr() for t in ts)
        n = int(boxes.shape[0])
        e.first, e.R, e.chunk_first = first, n, chunk
        e.G = 0 if gtb is None else int(gtb.shape[0])
        e.height, e.width = (0.0, 0.0) if size is None else (float(size[0]), float(size[1]))
        first += n
        chunk += _chunks(n)
    return T.upload(tab, len(images), dev)[0], hold, first, chunk


# ------------------------------------------------------------------------------------------------------------------ match and label
def match_and_label(proposals, targets, iou_threshold, num_classes=1, *, stats=None, _phase_ms=None):
    """The reference's CustomCascadeROIHeads._match_and_label_boxes for one cascade stage, in one launch for the whole batch.

    proposals: one item per image, a dict or an object with `proposal_boxes` float32 [R_i,4] XYXY (`.tensor` unwrapped), or the tensor
    itself.  targets: one item per image with `gt_boxes` float32 [G_i,4], `gt_classes` integer [G_i], `gt_scores` float32 [G_i] (and
    optionally `gt_masks`, which is passed through).  Detectron2's pairwise_iou in float32, every operation rounded on its own (equal
    bit for bit to a float32 NumPy restatement), then Matcher([iou_threshold], [0, 1], allow_low_quality_matches=False): per proposal
    the maximum over the image's ground truths, the LOWEST index that attains it (what torch's CPU max(dim=0) returns), foreground iff
    the maximum >= iou_threshold.

    Returns a list with one dict per image, every tensor a view into a flat buffer of all R proposals: `proposal_boxes` (the input),
    `matched_idxs` int64, `matched_vals` float32, `gt_classes` int64 (the matched class, num_classes on background rows), `gt_boxes`
    [R_i,4] and `gt_scores` [R_i] (gathered by matched_idxs on EVERY row, background included, as the reference does), `mask_index`
    (the same tensor as matched_idxs: mask_loss.mask_rcnn_loss_weighted reads `gt_masks` through it) and `gt_masks` when the target has
    them.

    Where this departs from the reference, on purpose:
      * an image without ground truths: every row is background with zero gt_boxes AND zero gt_scores.  The reference leaves
        `gt_scores` unbound on that branch (custom_cascade_rcnn.py:289-299 assigns gt_weights instead) and raises, or silently reuses
        the previous image's scores; that bug is not reproduced.
      * a proposal with a non-finite coordinate is counted in `bad` and labelled background (index 0, value 0).  Detectron2's Matcher
        would leave a NaN IoU at its default label 1, foreground.
      * a NaN IoU that comes from a GROUND TRUTH (a non-finite coordinate, or areas that overflow) never wins the maximum, where torch's
        max would hand it on and the Matcher would again label the row 1: the row is matched among its other ground truths, and a row
        whose every IoU is NaN is background with index 0 and value 0.  Such rows are not counted; ground truths are the caller's.

    stats: a dict that receives `num_fg`, `num_bg` and `bad`, int32 [N] tensors ON THE DEVICE, and `scalars`, a function that gives the
    two logged means (stage{k}/roi_head/num_fg_samples, num_bg_samples) and reads the device only when it is called.  The call itself
    never reads the device back; like mask_loss, it uploads its table of images with one blocking host-to-device copy.  ValueError for argument errors before any launch, RuntimeError off the GPU."""
    proposals, targets = list(proposals), list(targets)
    if len(proposals) != len(targets) or not proposals:
        raise ValueError(f"box_loss: match_and_label needs one target per image and at least one image, got {len(proposals)} and {len(targets)}")
    if not isinstance(num_classes, int) or num_classes < 0:
        raise ValueError(f"box_loss: num_classes must be a non-negative integer, got {num_classes!r}")
    t = float(iou_threshold)
    if math.isnan(t):
        raise ValueError("box_loss: the IoU threshold is NaN")
    images, masks, tensors = [], [], []
    for k, (p, g) in enumerate(zip(proposals, targets)):
        boxes = T.unwrap(p if isinstance(p, torch.Tensor) else T.getter(p)("proposal_boxes"))
        _check_boxes(boxes, f"proposals[{k}]", "proposal_boxes")
        get = T.getter(g)
        gtb, gtc, gts = T.unwrap(get("gt_boxes")), get("gt_classes"), get("gt_scores")
        n = _check_boxes(gtb, f"targets[{k}]", "gt_boxes")
        _check_vector(gtc, n, f"targets[{k}]", "gt_classes", True)
        _check_vector(gts, n, f"targets[{k}]", "gt_scores", False)
        images.append((boxes, gtb, gtc, gts, None))
        masks.append(get("gt_masks"))
        tensors += [boxes, gtb, gtc, gts]
    R = sum(int(im[0].shape[0]) for im in images)
    if R >= 1 << 31:
        raise ValueError("box_loss: 2^31 proposals or more")
    dev = _device(tensors, "match_and_label")
    N = len(images)
    with torch.cuda.device(dev):
        images = [(b, gb, gc.to(torch.int64), gs, s) for b, gb, gc, gs, s in images]
        idx = torch.empty(R, dtype=torch.int64, device=dev)
        vals, scores = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
        classes, boxes = torch.empty(R, dtype=torch.int64, device=dev), torch.empty((R, 4), dtype=torch.float32, device=dev)
        counts = torch.zeros((3, N), dtype=torch.int32, device=dev)
        if R:
            buf, hold, _, n_chunks = _upload_table(images, dev)
            T.timed(lambda _: L.check(L.lib().umr_box_match(_p(buf), N, R, n_chunks, t, num_classes, _p(idx), _p(vals), _p(classes), _p(boxes),
                                                            _p(scores), _p(counts), _stream()), "umr_box_match"),
                    (("match", 1),), _phase_ms)                                # tools/box_loss_bench.py times the launch
            del hold
    sizes = [int(im[0].shape[0]) for im in images]
    out = []
    for k, parts in enumerate(zip(idx.split(sizes), vals.split(sizes), classes.split(sizes), boxes.split(sizes), scores.split(sizes))):
        i, v, c, b, s = parts
        item = {"proposal_boxes": images[k][0], "matched_idxs": i, "matched_vals": v, "gt_classes": c, "gt_boxes": b, "gt_scores": s,
                "mask_index": i}
        if masks[k] is not None:
            item["gt_masks"] = masks[k]
        out.append(item)
    if stats is not None:
        def scalars(values=None):
            c = (counts if values is None else values).tolist()
            return {"num_fg_samples": sum(c[0]) / N, "num_bg_samples": sum(c[1]) / N, "bad": int(sum(c[2]))}
        stats["num_fg"], stats["num_bg"], stats["bad"], stats["counts"], stats["scalars"] = counts[0], counts[1], counts[2], counts, scalars
    return out


# ------------------------------------------------------------------------------------------------------------------ the transforms
def _check_deltas(d, n, name="proposal_deltas"):
    if not isinstance(d, torch.Tensor) or d.dtype not in (torch.float32, torch.bfloat16) or d.dim() != 2 or d.shape[1] != 4:
        raise ValueError(f"box_loss: {name} must be float32 or bfloat16 [R, 4] (class-agnostic), got {getattr(d, 'dtype', type(d))} "
                         f"{list(getattr(d, 'shape', []))}")
    if n is not None and d.shape[0] != n:
        raise ValueError(f"box_loss: {int(d.shape[0])} rows of {name} for {n} proposals")


def apply_deltas(deltas, boxes, weights):
    """Detectron2's Box2BoxTransform(weights).apply_deltas(deltas, boxes), class-agnostic, in float32: deltas float32 or bfloat16 [n,4],
    boxes float32 [n,4] XYXY -> float32 [n,4].  dw and dh are clamped at log(1000 / 16); expf, not a fast intrinsic."""
    boxes = T.unwrap(boxes)
    n = _check_boxes(boxes, "apply_deltas", "boxes")
    _check_deltas(deltas, n, "deltas")
    w = _weights4(weights)
    dev = _device([deltas, boxes], "apply_deltas")
    with torch.cuda.device(dev):
        d, b = deltas.detach().contiguous(), boxes.contiguous()
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        L.check(L.lib().umr_box_apply_deltas(_p(d), T.dtype_code(d), _p(b), n, *w, _p(out), _stream()), "umr_box_apply_deltas")
    return out


def get_deltas(src_boxes, target_boxes, weights):
    """Detectron2's Box2BoxTransform(weights).get_deltas(src_boxes, target_boxes) in float32: two float32 [n,4] -> float32 [n,4].
    Detectron2 asserts positive source widths; this plain op returns what the arithmetic gives (inf / NaN there)."""
    src, tgt = T.unwrap(src_boxes), T.unwrap(target_boxes)
    n = _check_boxes(src, "get_deltas", "src_boxes")
    if _check_boxes(tgt, "get_deltas", "target_boxes") != n:
        raise ValueError(f"box_loss: get_deltas: {n} source boxes for {int(tgt.shape[0])} target boxes")
    w = _weights4(weights)
    dev = _device([src, tgt], "get_deltas")
    with torch.cuda.device(dev):
        s, t = src.contiguous(), tgt.contiguous()
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        L.check(L.lib().umr_box_get_deltas(_p(s), _p(t), n, *w, _p(out), _stream()), "umr_box_get_deltas")
    return out


def _proposal_boxes(proposals):
    out = []
    for k, p in enumerate(proposals):
        b = T.unwrap(p if isinstance(p, torch.Tensor) else T.getter(p)("proposal_boxes"))
        _check_boxes(b, f"proposals[{k}]", "proposal_boxes")
        out.append(b)
    return out


def next_stage_proposals(proposal_deltas, proposals, box2box_weights, image_sizes, training=True, *, _phase_ms=None):
    """FastRCNNOutputLayers.predict_boxes + CustomCascadeROIHeads._create_proposals_from_boxes: the stage's deltas applied to its
    proposals (apply_deltas), Boxes.clip to each image's (height, width) and, in training, only the boxes that are nonempty() (width > 0
    and height > 0), compacted in order.  proposal_deltas: float32 or bfloat16 [R,4]; proposals: one item per image with
    `proposal_boxes` float32 [R_i,4] (or the tensors); image_sizes: one (h, w) per image.

    Returns (boxes float32 [R,4], keep bool [R], counts int32 [N]), all on the device: the kept boxes of image 0, then of image 1, ...
    in their order, the rows past counts.sum() undefined; at inference nothing is dropped and counts are the R_i.  The caller reads
    `counts` once when it needs Python lengths (`split_proposals`).  Two launches and the blocking upload of the table; nothing is read back.  The result carries no gradient,
    as in the reference (`b.detach()`)."""
    boxes = _proposal_boxes(list(proposals))
    sizes = [tuple(float(v) for v in s) for s in image_sizes]
    if len(sizes) != len(boxes) or not boxes or any(len(s) != 2 or not all(math.isfinite(v) and v >= 0 for v in s) for s in sizes):
        raise ValueError("box_loss: next_stage_proposals needs one finite, non-negative (h, w) per image and at least one image")
    R = sum(int(b.shape[0]) for b in boxes)
    _check_deltas(proposal_deltas, R)
    w = _weights4(box2box_weights)
    dev = _device([proposal_deltas] + boxes, "next_stage_proposals")
    N = len(boxes)
    with torch.cuda.device(dev):
        out = torch.empty((R, 4), dtype=torch.float32, device=dev)
        keep = torch.empty(R, dtype=torch.uint8, device=dev)
        counts = torch.zeros(N, dtype=torch.int32, device=dev)
        if R:
            d = proposal_deltas.detach().contiguous()
            buf, hold, _, n_chunks = _upload_table([(b, None, None, None, s) for b, s in zip(boxes, sizes)], dev)
            nbytes = L.lib().umr_box_decode_workspace(R, n_chunks)
            ws = T.workspace(nbytes, dev)
            T.timed(lambda _: L.check(L.lib().umr_box_decode(_p(buf), N, R, n_chunks, _p(d), T.dtype_code(d), *w, int(bool(training)), _p(out),
                                                             _p(keep), _p(counts), _p(ws), nbytes, _stream()), "umr_box_decode"),
                    (("decode", 1),), _phase_ms)
            del hold
    return out, keep.view(torch.bool), counts


def split_proposals(boxes, counts):
    """the per-image views of next_stage_proposals' compacted boxes; reads `counts` (one synchronisation)"""
    n = [int(v) for v in counts.tolist()]
    return list(boxes[:sum(n)].split(n))


# ------------------------------------------------------------------------------------------------------------------ weights and losses
def _loss_images(proposals, need_classes, need_scores):
    images, tensors = [], []
    for k, p in enumerate(proposals):
        get = T.getter(p)
        boxes, gtb = T.unwrap(get("proposal_boxes")), T.unwrap(get("gt_boxes"))
        n = _check_boxes(boxes, f"proposals[{k}]", "proposal_boxes")
        if _check_boxes(gtb, f"proposals[{k}]", "gt_boxes") != n:
            raise ValueError(f"box_loss: proposals[{k}]: {int(gtb.shape[0])} matched gt_boxes for {n} proposals")
        gtc = gts = None
        if need_classes:
            gtc = get("gt_classes")
            _check_vector(gtc, n, f"proposals[{k}]", "gt_classes", True)
        if need_scores:
            gts = get("gt_scores")
            _check_vector(gts, n, f"proposals[{k}]", "gt_scores", False)
        images.append((boxes, gtb, gtc, gts, None))
        tensors += [t for t in (boxes, gtb, gtc, gts) if t is not None]
    return images, tensors


def _check_droploss(droploss, N):
    try:
        thresh, single = droploss
        thresh = float(thresh)
    except (TypeError, ValueError):
        raise ValueError("box_loss: droploss must be (iou_thresh, is_single_object) or None") from None
    if math.isnan(thresh):
        raise ValueError("box_loss: the drop-loss IoU threshold is NaN")
    if single is not None and (not isinstance(single, torch.Tensor) or tuple(single.shape) != (N,) or single.dtype.is_complex):
        raise ValueError(f"box_loss: is_single_object must be a [{N}] tensor or None, got {getattr(single, 'dtype', type(single))} "
                         f"{list(getattr(single, 'shape', []))}")
    return thresh, single


def droploss_weights(proposal_deltas, proposals, box2box_weights, iou_thresh, is_single_object=None):
    """The weights of the reference's drop-loss block (custom_cascade_rcnn.py:195-230) for one stage: float32 [R] of 0 / 1, on the device,
    one launch, no torch.unique and nothing read back.  proposals: one item per image with `proposal_boxes` and the MATCHED `gt_boxes`
    [R_i,4] (match_and_label's output).  The reference is reproduced with its quirks:
      * the ground-truth set of image i is the first n_i rows of its matched gt_boxes, where n_i is the number of distinct rows among
        its first min(100, R_i) -- the reference counts with torch.unique(x.gt_boxes.tensor[:100], dim=0) but then SLICES the un-uniqued
        tensor, so the set may hold duplicates and miss ground truths that first appear further down;
      * the predicted box is apply_deltas of the stage's own deltas on its proposals, unclipped;
      * iou_max = pairwise_iou_max_scores over that set (Detectron2's IoU formula); the weight is 0 where iou_max <= iou_thresh, else 1
        (a NaN keeps the row);
      * afterwards row r of the flat batch takes weight 1 where is_single_object[r // (R // N)] == 1 (for r // (R // N) < N): the
        reference fills its indicator BY POSITION, assuming R // N rows per image, not by the image the row belongs to.
    is_single_object: a [N] tensor or None."""
    proposals = list(proposals)
    images, tensors = _loss_images(proposals, False, False)
    if not images:
        raise ValueError("box_loss: droploss_weights needs at least one image")
    R = sum(int(im[0].shape[0]) for im in images)
    _check_deltas(proposal_deltas, R)
    w = _weights4(box2box_weights)
    thresh, single = _check_droploss((iou_thresh, is_single_object), len(images))
    dev = _device([proposal_deltas] + tensors + ([] if single is None else [single]), "droploss_weights")
    with torch.cuda.device(dev):
        out = torch.empty(R, dtype=torch.float32, device=dev)
        if R:
            d = proposal_deltas.detach().contiguous()
            s = None if single is None else single.to(torch.float32).contiguous()
            buf, hold, _, n_chunks = _upload_table(images, dev)
            L.check(L.lib().umr_box_drop_weights(_p(buf), len(images), R, n_chunks, _p(d), T.dtype_code(d), *w, thresh, _p(s), _p(out),
                                                 _stream()), "umr_box_drop_weights")
            del hold
    return out


class _BoxLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, deltas, run):
        loss_cls, loss_box, g_scores, g_deltas = run(scores.detach().contiguous(), deltas.detach().contiguous())
        ctx.save_for_backward(g_scores, g_deltas)
        return loss_cls, loss_box

    @staticmethod
    def backward(ctx, g_cls, g_box):
        g_scores, g_deltas = ctx.saved_tensors
        return g_scores * g_cls, g_deltas * g_box, None    # each saved gradient times its own incoming scalar, in the inputs' type


def fast_rcnn_losses(scores, proposal_deltas, proposals, *, box2box_weights, num_classes=1, smooth_l1_beta=0.0, use_soft_targets=True,
                     droploss=None, weights=None, loss_weight=1.0, box_reg_loss_type="smooth_l1", stats=None, _phase_ms=None):
    """The reference's FastRCNNOutputLayers.losses (fast_rcnn.py:329-390, 462-514) with the drop-loss block of
    CustomCascadeROIHeads._forward_box in front of it, as one differentiable call: one main launch and a finishing launch.

    scores [R, K+1] and proposal_deltas [R,4] (class-agnostic): float32 or bfloat16, the same type, on the GPU; K == num_classes.
    proposals: one item per image with `proposal_boxes` [R_i,4], and the matched `gt_boxes` [R_i,4], `gt_classes` integer [R_i] and
    (with soft targets) `gt_scores` float32 [R_i] -- match_and_label's output.

    Weights: droploss=None and weights=None give the unweighted losses (the reference's `no_gt_found` branch; the caller decides).
    droploss=(iou_thresh, is_single_object) computes droploss_weights(...) inside the same launch, quirks included (see there: the
    ground-truth set from the first 100 matched rows, the unclipped prediction, the single-object indicator by position).  weights=
    passes ready-made float32 [R] weights instead.

    loss_cls: with use_soft_targets the targets are (fg, 1 - fg), fg = gt_scores, zero where gt_classes == num_classes; this needs
    K + 1 == 2 (ValueError otherwise).  Per row -(fg * log_softmax_0 + (1 - fg) * log_softmax_1), times the row's weight, mean over R.
    Without soft targets the usual cross-entropy on gt_classes, same weights and mean.  loss_box_reg: over the rows with
    0 <= gt_classes < num_classes, fvcore's smooth_l1(pred - get_deltas(proposal, gt_box), beta) summed over the four coordinates
    (|d| when beta < 1e-5, else 0.5 d^2 / beta below beta and |d| - 0.5 beta above), times gt_scores with soft targets, the total
    divided by max(R, 1).  Only "smooth_l1" is supported.  Detectron2 asserts positive source widths; here a foreground row whose
    proposal or ground-truth extent is not positive or not finite contributes 0 and is counted in `bad`.  Arithmetic is float32 whatever
    the inputs' type, the sums are double in a fixed order: the same input gives the same bytes.

    Returns {"loss_cls", "loss_box_reg"}, 0-dim float32, each times loss_weight (a float, or a dict with those keys).  Both come from
    one torch.autograd.Function with two outputs: the main launch also writes d loss_cls / d scores = w_r (softmax - target) / R and
    d loss_box_reg / d deltas = sign(d) (or d / beta) * score / R, zero on background rows, in the inputs' types, and backward multiplies
    each by its incoming scalar.  R == 0 gives zero losses that are still attached to the graph.

    stats: a dict that receives `counters` -- int64 [7] ON THE DEVICE in the order of COUNTERS: rows, foreground rows, argmax == class,
    foreground with argmax == class, foreground predicted background, rows of weight 0, bad rows -- `scalars`, a function that turns them
    into the reference's logged `cls_accuracy`, `fg_cls_accuracy` and `false_negative` (the last two absent without foreground, as in the
    reference; nothing without rows) and reads the device only when called, and `weights`, the float32 [R] weights used.  The call never
    reads the device back (its table of images goes up in one blocking host-to-device copy, as mask_loss's does).  ValueError for argument errors before any launch; RuntimeError off the GPU."""
    if box_reg_loss_type != "smooth_l1":
        raise ValueError(f"box_loss: only the smooth_l1 box regression loss is supported, got {box_reg_loss_type!r}")
    x = scores
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"box_loss: scores must be float32 or bfloat16 [R, K + 1], got {getattr(x, 'dtype', type(x))} {list(getattr(x, 'shape', []))}")
    if not isinstance(num_classes, int) or num_classes < 1:
        raise ValueError(f"box_loss: num_classes must be a positive integer, got {num_classes!r}")
    R, K1 = int(x.shape[0]), int(x.shape[1])
    if K1 != num_classes + 1:
        raise ValueError(f"box_loss: {K1} columns of scores for {num_classes} classes and the background")
    if use_soft_targets and K1 != 2:
        raise ValueError(f"box_loss: soft targets need K + 1 == 2 columns (foreground, background), got {K1}")
    _check_deltas(proposal_deltas, R)
    if proposal_deltas.dtype != x.dtype:
        raise ValueError(f"box_loss: scores are {x.dtype} and proposal_deltas {proposal_deltas.dtype}")
    beta = float(smooth_l1_beta)
    if not beta >= 0 or math.isinf(beta):
        raise ValueError(f"box_loss: smooth_l1_beta must be finite and >= 0, got {smooth_l1_beta!r}")
    bw = _weights4(box2box_weights)
    proposals = list(proposals)
    images, tensors = _loss_images(proposals, True, bool(use_soft_targets))
    total = sum(int(im[0].shape[0]) for im in images)
    if total != R:
        raise ValueError(f"box_loss: {R} rows of scores for {total} proposals")
    if R >= 1 << 31:
        raise ValueError("box_loss: 2^31 proposals or more")
    if droploss is not None and weights is not None:
        raise ValueError("box_loss: pass droploss= or weights=, not both")
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (R,)):
        raise ValueError(f"box_loss: weights must be float32 [{R}], got {getattr(weights, 'dtype', type(weights))} "
                         f"{list(getattr(weights, 'shape', []))}")
    thresh, single = (0.0, None) if droploss is None else _check_droploss(droploss, len(images))
    if isinstance(loss_weight, dict):
        lw = {k: float(loss_weight.get(k, 1.0)) for k in ("loss_cls", "loss_box_reg")}
    else:
        lw = {k: float(loss_weight) for k in ("loss_cls", "loss_box_reg")}
    dev = _device([x, proposal_deltas] + tensors + [t for t in (weights, single) if t is not None], "fast_rcnn_losses")
    mode = 2 if droploss is not None else (1 if weights is not None else 0)
    N = len(images)
    got = {}

    def run(s, d):
        with torch.cuda.device(dev):
            loss_cls, loss_box = torch.zeros((), dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.float32, device=dev)
            counters = torch.zeros(7, dtype=torch.int64, device=dev)
            g_s, g_d = torch.empty_like(s), torch.empty_like(d)
            w_out = torch.empty(R, dtype=torch.float32, device=dev)
            got["counters"], got["weights"] = counters, w_out
            if R == 0:
                return loss_cls, loss_box, g_s, g_d
            table = [(b, gb, gc.to(torch.int64), gs, sz) for b, gb, gc, gs, sz in images]
            buf, hold, _, n_chunks = _upload_table(table, dev)
            nbytes = L.lib().umr_box_loss_workspace(n_chunks)
            ws = T.workspace(nbytes, dev)
            w_in = None if weights is None else weights.detach().contiguous()
            sg = None if single is None else single.to(torch.float32).contiguous()

            def launch(phases):
                L.check(L.lib().umr_box_loss(_p(buf), N, R, n_chunks, K1, num_classes, _p(s), _p(d), T.dtype_code(s), *bw, beta,
                                             int(bool(use_soft_targets)), mode, thresh, _p(w_in), _p(sg), phases, _p(w_out), _p(g_s), _p(g_d),
                                             _p(loss_cls), _p(loss_box), _p(counters), _p(ws), nbytes, _stream()), "umr_box_loss")
            T.timed(launch, (("loss_main", 1), ("loss_finish", 2)), _phase_ms)
            del hold
        return loss_cls, loss_box, g_s, g_d

    loss_cls, loss_box = _BoxLoss.apply(x, proposal_deltas, run)
    out = {"loss_cls": loss_cls if lw["loss_cls"] == 1.0 else loss_cls * lw["loss_cls"],
           "loss_box_reg": loss_box if lw["loss_box_reg"] == 1.0 else loss_box * lw["loss_box_reg"]}
    if stats is not None:
        counters = got["counters"]

        def scalars(values=None):
            rows, fg, acc, fg_acc, fn, dropped, bad = (int(v) for v in (counters if values is None else values).tolist())
            s = {"dropped": dropped, "bad": bad}
            if rows:
                s["cls_accuracy"] = acc / rows
                if fg:
                    s["fg_cls_accuracy"], s["false_negative"] = fg_acc / fg, fn / fg
            return s
        stats["counters"], stats["scalars"], stats["weights"] = counters, scalars, got["weights"]
    return out
