"""The plain restatement of unmore_amd.box_loss for the tests: NumPy in float32 or float64 for IoU, matching, the two box transforms,
decode / clip / compaction and the drop-loss weights; torch CPU float64 autograd for the two losses; a seeded ragged-batch generator;
the loader of tests/golden/box_loss.npz.  Written from the formulas of Detectron2's pairwise_iou, Matcher, Box2BoxTransform and
Boxes.clip / nonempty, fvcore's smooth_l1_loss and the reference's custom_cascade_rcnn.py / fast_rcnn.py; every operation is one NumPy
ufunc on arrays of `dtype`, so the float32 run rounds after every operation as the kernels do."""
import math
import os

import numpy as np
import torch

SCALE_CLAMP = math.log(1000.0 / 16)
UNIQUE_ROWS = 100
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_loss.npz")
STAGE_IOUS = (0.5, 0.6, 0.7)
STAGE_WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))


# ---------------------------------------------------------------------------------------------------------------- IoU and the matcher
def area_np(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def pairwise_iou_np(boxes1, boxes2, dtype=np.float32):
    """Detectron2's pairwise_iou(boxes1 [N,4], boxes2 [M,4]) -> [N,M]"""
    b1, b2 = np.asarray(boxes1, dtype=dtype).reshape(-1, 4), np.asarray(boxes2, dtype=dtype).reshape(-1, 4)
    a1, a2 = area_np(b1), area_np(b2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        wh = np.minimum(b1[:, None, 2:], b2[None, :, 2:]) - np.maximum(b1[:, None, :2], b2[None, :, :2])
        wh = np.where(wh > 0, wh, dtype(0))
        inter = wh[..., 0] * wh[..., 1]
        union = (a1[:, None] + a2[None, :]) - inter
        iou = np.where(inter > 0, inter / np.where(inter > 0, union, dtype(1)), dtype(0))
    return iou.astype(dtype)


def match_np(proposal_boxes, gt_boxes, gt_classes, gt_scores, threshold, num_classes=1, dtype=np.float32):
    """_match_and_label_boxes for one image with unmore_amd.box_loss.match_and_label's two written-down deviations (no ground truths:
    zero gt_scores; a non-finite proposal: bad, background, index 0, value 0).  A dict of arrays."""
    p = np.asarray(proposal_boxes, dtype=dtype).reshape(-1, 4)
    g = np.asarray(gt_boxes, dtype=dtype).reshape(-1, 4)
    n, G = len(p), len(g)
    bad = ~np.isfinite(p).all(axis=1)
    idx, vals = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=dtype)
    if G and n:
        iou = pairwise_iou_np(g, np.where(bad[:, None], dtype(0), p), dtype)          # [G, n]
        idx = iou.argmax(axis=0).astype(np.int64)                                    # the first maximum, as torch's CPU max(dim=0)
        vals = iou.max(axis=0)
        idx[bad], vals[bad] = 0, 0
    labels = (vals >= dtype(threshold)) & ~bad & (G > 0)
    if G:
        classes = np.where(labels, np.asarray(gt_classes, dtype=np.int64)[idx], num_classes)
        boxes, scores = np.asarray(gt_boxes, dtype=np.float32)[idx], np.asarray(gt_scores, dtype=np.float32)[idx]
    else:
        classes, boxes, scores = np.full(n, num_classes, dtype=np.int64), np.zeros((n, 4), dtype=np.float32), np.zeros(n, dtype=np.float32)
    return {"matched_idxs": idx, "matched_vals": vals, "labels": labels, "gt_classes": classes, "gt_boxes": boxes, "gt_scores": scores,
            "num_fg": int(labels.sum()), "num_bg": int(n - labels.sum()), "bad": int(bad.sum())}


# ---------------------------------------------------------------------------------------------------------------- the transforms
def apply_deltas_np(deltas, boxes, weights, dtype=np.float32):
    d, b = np.asarray(deltas, dtype=dtype).reshape(-1, 4), np.asarray(boxes, dtype=dtype).reshape(-1, 4)
    wx, wy, ww, wh = (dtype(v) for v in weights)
    half, clamp = dtype(0.5), dtype(np.float32(SCALE_CLAMP) if dtype == np.float32 else SCALE_CLAMP)
    with np.errstate(invalid="ignore", over="ignore"):
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        cx, cy = b[:, 0] + half * w, b[:, 1] + half * h
        dx, dy = d[:, 0] / wx, d[:, 1] / wy
        dw, dh = d[:, 2] / ww, d[:, 3] / wh
        dw, dh = np.where(dw > clamp, clamp, dw), np.where(dh > clamp, clamp, dh)
        pcx, pcy = dx * w + cx, dy * h + cy
        pw, ph = np.exp(dw) * w, np.exp(dh) * h
        out = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], axis=1)
    return out.astype(dtype)


def get_deltas_np(src, target, weights, dtype=np.float32):
    s, t = np.asarray(src, dtype=dtype).reshape(-1, 4), np.asarray(target, dtype=dtype).reshape(-1, 4)
    wx, wy, ww, wh = (dtype(v) for v in weights)
    half = dtype(0.5)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sw, sh = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
        scx, scy = s[:, 0] + half * sw, s[:, 1] + half * sh
        tw, th = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
        tcx, tcy = t[:, 0] + half * tw, t[:, 1] + half * th
        out = np.stack([wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * np.log(tw / sw), wh * np.log(th / sh)], axis=1)
    return out.astype(dtype)


def clip_np(boxes, size, dtype=np.float32):
    h, w = dtype(size[0]), dtype(size[1])
    b = np.array(boxes, dtype=dtype).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        b[:, 0::2] = np.where(b[:, 0::2] < 0, dtype(0), np.where(b[:, 0::2] > w, w, b[:, 0::2]))
        b[:, 1::2] = np.where(b[:, 1::2] < 0, dtype(0), np.where(b[:, 1::2] > h, h, b[:, 1::2]))
    return b


def next_stage_np(deltas, proposal_boxes, weights, image_sizes, training=True, dtype=np.float32):
    """predict_boxes + _create_proposals_from_boxes over a batch: (the per-image clipped boxes before the drop, keep [R], counts [N])"""
    clipped, keep, counts, at = [], [], [], 0
    for boxes, size in zip(proposal_boxes, image_sizes):
        n = len(boxes)
        b = clip_np(apply_deltas_np(np.asarray(deltas)[at:at + n], boxes, weights, dtype), size, dtype)
        with np.errstate(invalid="ignore"):
            k = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0) if training else np.ones(n, dtype=bool)
        clipped.append(b)
        keep.append(k)
        counts.append(int(k.sum()))
        at += n
    return clipped, (np.concatenate(keep) if keep else np.zeros(0, dtype=bool)), np.array(counts, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- drop-loss weights
def distinct_rows(gt_boxes):
    """the reference's torch.unique(x.gt_boxes.tensor[:100], dim=0).size()[0]"""
    head = np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4)[:UNIQUE_ROWS]
    return len(np.unique(head, axis=0)) if len(head) else 0


def droploss_iou_max_np(deltas, proposal_boxes, matched_gt_boxes, weights, dtype=np.float32):
    """per row the reference's iou_max: pairwise_iou_max_scores(apply_deltas(deltas, proposals), gt_boxes[:n_i]) image by image"""
    out, at = [], 0
    for boxes, gtb in zip(proposal_boxes, matched_gt_boxes):
        n = len(boxes)
        if n:
            pred = apply_deltas_np(np.asarray(deltas)[at:at + n], boxes, weights, dtype)
            out.append(pairwise_iou_np(pred, np.asarray(gtb)[:distinct_rows(gtb)], dtype).max(axis=1))
        at += n
    return np.concatenate(out) if out else np.zeros(0, dtype=dtype)


def droploss_weights_np(iou_max, thresh, is_single_object, n_images):
    """weights from iou_max, then the single-object indicator by POSITION (custom_cascade_rcnn.py:196-199, 228-230)"""
    iou_max = np.asarray(iou_max)
    R = len(iou_max)
    w = 1.0 - (iou_max <= iou_max.dtype.type(thresh)).astype(np.float32)
    if is_single_object is not None:
        per = R // n_images
        ind = np.zeros(R, dtype=np.float32)
        for i in range(n_images):
            ind[i * per:(i + 1) * per] = float(is_single_object[i])
        w[ind == 1] = 1
    return w.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the two losses
def smooth_l1_t(x, target, beta):
    """fvcore.nn.smooth_l1_loss(reduction="none")"""
    if beta < 1e-5:
        return torch.abs(x - target)
    n = torch.abs(x - target)
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def losses_reference(scores, deltas, proposal_boxes, gt_boxes, gt_classes, gt_scores, row_weights, box2box_weights, num_classes=1,
                     smooth_l1_beta=0.0, use_soft_targets=True, coef=(1.0, 1.0), dtype=torch.float64):
    """FastRCNNOutputLayers.losses on flat arrays in `dtype` with torch CPU autograd: (loss_cls, loss_box_reg, d(coef . losses)/d scores,
    d / d deltas, counters [7] in unmore_amd.box_loss.COUNTERS order).  Foreground rows whose proposal or ground-truth extent is not
    positive or finite add no box term and are counted bad, as the kernel documents."""
    s = torch.tensor(np.asarray(scores, dtype=np.float64), dtype=dtype, requires_grad=True)
    d = torch.tensor(np.asarray(deltas, dtype=np.float64), dtype=dtype, requires_grad=True)
    R, K1 = s.shape
    gc = torch.tensor(np.asarray(gt_classes, dtype=np.int64))
    w = torch.ones(R, dtype=dtype) if row_weights is None else torch.tensor(np.asarray(row_weights, dtype=np.float64), dtype=dtype)
    sc = torch.ones(R, dtype=dtype) if not use_soft_targets else torch.tensor(np.asarray(gt_scores, dtype=np.float64), dtype=dtype)
    logp = torch.log_softmax(s, dim=1)
    if use_soft_targets:
        fg_prob = sc.clone()
        fg_prob[gc == num_classes] = 0.0
        ce = -(fg_prob * logp[:, 0] + (1 - fg_prob) * logp[:, 1])
    else:
        ce = -logp[torch.arange(R), gc]
    loss_cls = (w * ce).mean() if R else s.sum() * 0
    fg = (gc >= 0) & (gc < num_classes)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    tgt = get_deltas_np(proposal_boxes, gt_boxes, box2box_weights, np_dtype)
    p, g = np.asarray(proposal_boxes, dtype=np.float64).reshape(-1, 4), np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
    ok = (p[:, 2] - p[:, 0] > 0) & (p[:, 3] - p[:, 1] > 0) & (g[:, 2] - g[:, 0] > 0) & (g[:, 3] - g[:, 1] > 0) & np.isfinite(tgt).all(axis=1)
    use = fg & torch.from_numpy(ok)
    t = torch.tensor(np.where(ok[:, None], tgt, 0.0), dtype=dtype)
    loss_box = (smooth_l1_t(d[use], t[use], smooth_l1_beta) * sc[use, None]).sum() / max(R, 1.0)
    (coef[0] * loss_cls + coef[1] * loss_box).backward()
    pred = s.detach().argmax(dim=1) if R else torch.zeros(0, dtype=torch.int64)
    counters = [R, int(fg.sum()), int((pred == gc).sum()), int((pred[fg] == gc[fg]).sum()), int((pred[fg] == K1 - 1).sum()),
                int((w == 0).sum()), int((fg & ~torch.from_numpy(ok)).sum())]
    gs = s.grad if s.grad is not None else torch.zeros_like(s)
    gd = d.grad if d.grad is not None else torch.zeros_like(d)
    return float(loss_cls.detach()), float(loss_box.detach()), gs.numpy(), gd.numpy(), counters


def logged_scalars(counters):
    rows, fg, acc, fg_acc, fn = (int(v) for v in counters[:5])
    s = {}
    if rows:
        s["cls_accuracy"] = acc / rows
        if fg:
            s["fg_cls_accuracy"], s["false_negative"] = fg_acc / fg, fn / fg
    return s


# ---------------------------------------------------------------------------------------------------------------- batches
def ragged_batch(seed, proposals_per_image, gts_per_image, sizes, box_scale=0.25):
    """A seeded ragged batch: per image ground truths of about box_scale of the frame with classes 0 and scores in [0.2, 1] (the first
    two scores of an image are 0 and 1), proposals that are jittered ground truths, exact duplicates of them, boxes touching one, and
    uniform boxes.  Lists of float32 arrays."""
    rng = np.random.RandomState(seed)
    images = []
    for n, G, (h, w) in zip(proposals_per_image, gts_per_image, sizes):
        cx, cy = rng.uniform(0, w, G), rng.uniform(0, h, G)
        bw, bh = rng.uniform(0.3, 1.0, G) * box_scale * w, rng.uniform(0.3, 1.0, G) * box_scale * h
        gt = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=1).astype(np.float32).reshape(-1, 4)
        scores = rng.uniform(0.2, 1.0, G).astype(np.float32)
        scores[:2] = np.array([0.0, 1.0], dtype=np.float32)[:G]
        props = np.zeros((n, 4), dtype=np.float32)
        for j in range(n):
            kind = rng.randint(4) if G else 3
            g = gt[rng.randint(G)] if G else None
            if kind == 0:                                                           # a jittered ground truth
                props[j] = g + rng.uniform(-0.25, 0.25, 4).astype(np.float32) * np.array([g[2] - g[0], g[3] - g[1]] * 2, dtype=np.float32)
            elif kind == 1:                                                         # an exact duplicate
                props[j] = g
            elif kind == 2:                                                         # touching it on the right: intersection of zero width
                props[j] = [g[2], g[1], g[2] + (g[2] - g[0]), g[3]]
            else:
                x, y = rng.uniform(-0.1 * w, w), rng.uniform(-0.1 * h, h)
                props[j] = [x, y, x + rng.uniform(0.05, 0.5) * w, y + rng.uniform(0.05, 0.5) * h]
        images.append({"proposal_boxes": props, "gt_boxes": gt, "gt_classes": np.zeros(G, dtype=np.int64), "gt_scores": scores,
                       "image_size": (h, w)})
    return images


def load_fixture(path=GOLDEN):
    z = np.load(path)
    return {k: z[k] for k in z.files}
