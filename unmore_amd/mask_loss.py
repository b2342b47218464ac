"""Mask-head targets and the score-weighted mask loss of the stage-3 detector on the device (cad/modeling/roi_heads/roi_heads.py:963-1045,
mask_rcnn_loss_weighted, called from CustomMaskRCNNConvUpsampleHead.forward :1172-1197 under the recipe's USE_SOFT_TARGETS): for every
foreground proposal the matched ground-truth mask is cropped and resized to the head's resolution (Detectron2's
BitMasks.crop_and_resize: ROIAlign with an adaptive sample grid, then >= 0.5) and a binary cross-entropy against the head's logits is
weighted by the pseudo-label's score.  `mask_targets` makes the targets alone; `mask_rcnn_loss_weighted` / `mask_rcnn_loss` do targets,
loss, the logged counters and the gradient in one sequence of launches (csrc/mask_loss.hip).  The masks are read in place through
`mask_index`: the reference's gather of one full frame per proposal (`gt_masks[matched_idxs]`) is never made.  No CPU fallback:
tests/mask_loss_common.py restates the method in NumPy and torch CPU ops."""
import torch

from . import _lib as L
from . import _tables as T
from .ops import _p, _stream

MAX_SIDE = 512
MAX_LDS_BYTES = 160 * 1024
COUNTERS = ("incorrect", "positive", "false_positive", "false_negative", "bad")


def _lds_bytes(side, max_h, max_w):
    return 16 * (max_h + max_w) + 32 * side + 328        # csrc/mask_loss.hip: ml_lds_bytes


def _fields(item, k):
    """(masks, boxes, mask_index, gt_classes) of one image: a dict or an object with Detectron2's Instances fields"""
    get = T.getter(item)
    masks, boxes = get("gt_masks"), get("proposal_boxes")
    if masks is None or boxes is None:
        raise ValueError(f"mask_loss: instances[{k}] needs gt_masks and proposal_boxes")
    index, classes = get("mask_index"), get("gt_classes")
    return T.unwrap(masks), T.unwrap(boxes), index, classes


def _check_image(masks, boxes, index, what):
    """shape and dtype checks of one image, without touching its data: R_i"""
    if not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.bool, torch.uint8) or masks.dim() != 3 or masks.shape[1] < 1 \
            or masks.shape[2] < 1:
        raise ValueError(f"mask_loss: {what}: masks must be bool or uint8 [G, H, W] with H, W >= 1, got "
                         f"{getattr(masks, 'dtype', type(masks))} {list(getattr(masks, 'shape', []))}")
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError(f"mask_loss: {what}: boxes must be float32 [R, 4], got {getattr(boxes, 'dtype', type(boxes))} "
                         f"{list(getattr(boxes, 'shape', []))}")
    n = int(boxes.shape[0])
    if index is None:
        if n != masks.shape[0]:
            raise ValueError(f"mask_loss: {what}: {n} boxes for {masks.shape[0]} masks and no mask_index")
    elif not isinstance(index, torch.Tensor) or index.dtype not in (torch.int32, torch.int64) or tuple(index.shape) != (n,):
        raise ValueError(f"mask_loss: {what}: mask_index must be int32 or int64 [{n}], got {getattr(index, 'dtype', type(index))} "
                         f"{list(getattr(index, 'shape', []))}")
    if masks.shape[1] * masks.shape[2] >= 1 << 31:
        raise ValueError(f"mask_loss: {what}: a frame of 2^31 pixels or more")
    return n


def _check_side(side, images):
    if not isinstance(side, int) or side < 1 or side > MAX_SIDE:
        raise ValueError(f"mask_loss: the side must be an integer in [1, {MAX_SIDE}], got {side!r}")
    max_h = max([int(m.shape[1]) for m, _, _ in images], default=1)
    max_w = max([int(m.shape[2]) for m, _, _ in images], default=1)
    if _lds_bytes(side, max_h, max_w) > MAX_LDS_BYTES:
        raise ValueError(f"mask_loss: the sample tables of a {max_h} x {max_w} frame at side {side} take {_lds_bytes(side, max_h, max_w)} bytes "
                         f"of LDS, more than {MAX_LDS_BYTES}")
    return max_h, max_w


def _device(tensors, what):
    return T.one_device(tensors, "mask_loss", what, " (mask_targets_np, loss_reference)")


def _upload_table(images, dev):
    """one umr_ml_image per image, in one host-to-device copy: (device buffer, what the table points into, R)"""
    tab = (L.MlImage * max(len(images), 1))()
    hold, first = [], 0
    for k, (masks, boxes, index) in enumerate(images):
        m, b = T.as_u8(masks), boxes.contiguous()
        i = None if index is None else index.contiguous()
        hold += [m, b, i]
        e = tab[k]
        e.masks, e.boxes, e.index = m.data_ptr(), b.data_ptr(), (None if i is None else i.data_ptr())
        e.H, e.W, e.G, e.first, e.R = int(m.shape[1]), int(m.shape[2]), int(m.shape[0]), first, int(b.shape[0])
        e.index64 = int(i is not None and i.dtype == torch.int64)
        first += int(b.shape[0])
    return T.upload(tab, len(images), dev)[0], hold, first


def mask_targets(masks, boxes, mask_index=None, side=28):
    """BitMasks.crop_and_resize(boxes, side) of masks[mask_index] on the device: bool [R, side, side].

    masks: bool or uint8 [G,H,W] (non-zero = set); boxes: float32 [R,4] XYXY; mask_index: int32 or int64 [R], None = the identity (then
    R == G).  Lists of each (mask_index: a list, or None for all) make a batch of images with their own sizes; the result is their
    targets in image order.  torchvision's roi_align(spatial_scale 1, sampling_ratio 0, aligned=True) of the float mask in float32,
    `>= 0.5`; csrc/mask_loss.hip writes the arithmetic out.  A proposal whose mask index is out of range, or whose box is not finite or
    beyond +-2^20, gets an empty target (mask_rcnn_loss_weighted counts those).  ValueError for argument errors before any launch,
    RuntimeError off the GPU."""
    if isinstance(masks, (list, tuple)):
        if not isinstance(boxes, (list, tuple)) or len(boxes) != len(masks) or (mask_index is not None and len(mask_index) != len(masks)):
            raise ValueError("mask_targets: a batch needs lists of equal length for masks, boxes and mask_index")
        images = [(m, b, None if mask_index is None else mask_index[k]) for k, (m, b) in enumerate(zip(masks, boxes))]
    else:
        images = [(masks, boxes, mask_index)]
    for k, (m, b, i) in enumerate(images):
        _check_image(m, b, i, f"image {k}")
    max_h, max_w = _check_side(side, images)
    if not images:
        raise ValueError("mask_targets: no image")
    dev = _device([t for im in images for t in im if t is not None], "mask_targets")
    with torch.cuda.device(dev):
        buf, hold, R = _upload_table(images, dev)
        out = torch.empty((R, side, side), dtype=torch.uint8, device=dev)
        if R:
            L.check(L.lib().umr_mask_targets(_p(buf), len(images), R, side, max_h, max_w, _p(out), _stream()), "umr_mask_targets")
    del hold
    return out.view(torch.bool)


def _run(logits, images, classes, weights, side, max_h, max_w, dev, want_targets, _phase_ms=None):
    """the launches: (loss f32 0-dim, grad like logits, counters int64 [5], targets bool or None)"""
    R, C = int(logits.shape[0]), int(logits.shape[1])
    with torch.cuda.device(dev):
        loss, counters = torch.zeros((), dtype=torch.float32, device=dev), torch.zeros(5, dtype=torch.int64, device=dev)
        grad = torch.empty_like(logits)
        targets = torch.empty((R, side, side), dtype=torch.uint8, device=dev) if want_targets else None
        if R == 0:
            return loss, grad, counters, (None if targets is None else targets.view(torch.bool))
        buf, hold, _ = _upload_table(images, dev)
        nbytes = L.lib().umr_mask_loss_workspace(R, side)
        ws = T.workspace(nbytes, dev)

        def launch(phases):
            L.check(L.lib().umr_mask_loss(_p(buf), len(images), R, C, side, max_h, max_w, _p(logits), T.dtype_code(logits), _p(classes),
                                          _p(weights), phases, _p(targets), _p(grad), _p(loss), _p(counters), _p(ws), nbytes, _stream()),
                    "umr_mask_loss")
        T.timed(launch, (("targets_loss", 1), ("finish", 2)), _phase_ms)     # tools/mask_loss_bench.py times the two parts
        del hold
    return loss, grad, counters, (None if targets is None else targets.view(torch.bool))


class _MaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, run):
        loss, grad = run(logits.detach().contiguous())
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None                              # the saved gradient times the incoming scalar, in the logits' type


def mask_rcnn_loss_weighted(pred_mask_logits, instances, weights=None, vis_period=0, *, stats=None, _phase_ms=None):
    """The reference's mask_rcnn_loss_weighted(pred_mask_logits, instances, weights) on the device, as one differentiable call.

    pred_mask_logits: [R,C,M,M] float32 or bfloat16 on the GPU, R = the proposals of all images in image order; C == 1 is the
    class-agnostic head, otherwise the channel of proposal r is gt_classes[r].  instances: one item per image, a dict (`gt_masks`
    bool or uint8 [G,H,W], `proposal_boxes` float32 [R_i,4] XYXY, optional `mask_index` int32 / int64 [R_i] -- without it R_i == G and
    mask r belongs to proposal r, as in the reference after its gather -- and `gt_classes` [R_i] when C > 1) or an object with
    Detectron2's fields (`.gt_masks.tensor`, `.proposal_boxes.tensor`, `.gt_classes`).  weights: float32 [R] (the pseudo-labels'
    scores); None gives Detectron2's unweighted mask_rcnn_loss.  vis_period: accepted for the reference's call sites and ignored (nothing
    is drawn).

    Returns the 0-dim float32 loss: the mean over R*M*M of w_r * bce_with_logits(x, target), terms in float32 whatever the logits'
    type.  It is a torch.autograd.Function: the gradient w_r * (sigmoid(x) - t) / (R*M*M) is written by the same launch, in the
    logits' type and zero in the other channels, and backward multiplies it by the incoming scalar.  R == 0 gives a zero loss that is
    still attached to the graph, and a zero gradient.

    stats: a dict that receives `counters` -- an int64 [5] tensor ON THE DEVICE, in the order of COUNTERS: elements with (x > 0) != target, positive targets,
    false positives, false negatives, and the number of bad proposals (mask index out of range, box not finite or beyond +-2^20, class
    out of range: they get an empty target) -- `scalars`, a function that turns the counters into the reference's logged `accuracy`,
    `false_positive` and `false_negative` (with its max(., 1.0) denominators) and `bad`; called without an argument it reads the
    device tensor, which is the only synchronisation and happens when the caller asks -- and `targets`, bool [R,M,M].  The call
    itself never synchronises.  ValueError for argument errors before any launch; RuntimeError off the GPU."""
    x = pred_mask_logits
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16) or x.shape[1] < 1:
        raise ValueError(f"mask_loss: logits must be float32 or bfloat16 [R, C, M, M], got {getattr(x, 'dtype', type(x))} "
                         f"{list(getattr(x, 'shape', []))}")
    if x.shape[2] != x.shape[3]:
        raise ValueError(f"mask_loss: Mask prediction must be square, got {list(x.shape)}")
    R, C, side = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    images, class_list = [], []
    for k, item in enumerate(instances):
        masks, boxes, index, cls = _fields(item, k)
        n = _check_image(masks, boxes, index, f"instances[{k}]")
        images.append((masks, boxes, index))
        if C > 1:
            if not isinstance(cls, torch.Tensor) or cls.dtype.is_floating_point or cls.dtype == torch.bool or tuple(cls.shape) != (n,):
                raise ValueError(f"mask_loss: instances[{k}]: {C} channels need integer gt_classes [{n}], got "
                                 f"{getattr(cls, 'dtype', type(cls))} {list(getattr(cls, 'shape', []))}")
            class_list.append(cls)
    total = sum(int(b.shape[0]) for _, b, _ in images)
    if total != R:
        raise ValueError(f"mask_loss: {R} rows of logits for {total} proposals")
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (R,)):
        raise ValueError(f"mask_loss: weights must be float32 [{R}], got {getattr(weights, 'dtype', type(weights))} "
                         f"{list(getattr(weights, 'shape', []))}")
    max_h, max_w = _check_side(side, images)
    if R >= 1 << 31:
        raise ValueError("mask_loss: 2^31 proposals or more")
    tensors = [x] + [t for im in images for t in im if t is not None] + class_list + ([] if weights is None else [weights])
    dev = _device(tensors, "mask_rcnn_loss_weighted")
    classes = torch.cat([c.to(torch.int64) for c in class_list]).contiguous() if class_list else None
    w = None if weights is None else weights.detach().contiguous()
    got = {}

    def run(logits):
        loss, grad, counters, targets = _run(logits, images, classes, w, side, max_h, max_w, dev, stats is not None, _phase_ms)
        got["counters"], got["targets"] = counters, targets
        return loss, grad

    loss = _MaskLoss.apply(x, run)
    if stats is not None:
        counters, n = got["counters"], float(R * side * side)

        def scalars(values=None):
            inc, pos, fp, fn, bad = (float(v) for v in (counters if values is None else values).tolist())
            return {"accuracy": 1 - inc / max(n, 1.0), "false_positive": fp / max(n - pos, 1.0), "false_negative": fn / max(pos, 1.0),
                    "bad": int(bad)}
        stats["counters"], stats["scalars"], stats["targets"] = counters, scalars, got["targets"]
    return loss


def mask_rcnn_loss(pred_mask_logits, instances, vis_period=0, *, stats=None):
    """Detectron2's unweighted mask_rcnn_loss: mask_rcnn_loss_weighted with weights of ones"""
    return mask_rcnn_loss_weighted(pred_mask_logits, instances, None, vis_period, stats=stats)
