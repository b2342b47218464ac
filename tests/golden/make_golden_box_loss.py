"""Generate tests/golden/box_loss.npz by running the REFERENCE's own box branch of CustomCascadeROIHeads on the CPU.

Run where the reference tree is at hand, never on the GPU box:
    python tests/golden/make_golden_box_loss.py /path/to/reference

What executes verbatim from the reference, read at generation time and compiled in a namespace of stand-ins; none of it is stored here:
  cad/structures/boxes.py                          the whole file (pairwise_iou_max_scores; it imports torch only)
  cad/modeling/box_regression.py                   _soft_dense_box_regression_loss
  cad/modeling/roi_heads/fast_rcnn.py              _log_classification_stats, and FastRCNNOutputLayers.losses / box_reg_loss / predict_boxes
  cad/modeling/roi_heads/custom_cascade_rcnn.py    CustomCascadeROIHeads._forward_box (its training branch), _match_and_label_boxes and
                                                   _create_proposals_from_boxes
The methods are cut out one by one (from `def` to the next `def` of the class) because their files import Detectron2 and fvcore, which
are absent.  _forward_box runs with a stand-in `self`: three stages, `_run_stage` returns predictions drawn here from a seeded generator
for the stage's number of proposals (and records them: they are the fixture's scores and deltas), `box_predictor[k]` is an object that
carries the recipe's settings and the three cut-out FastRCNNOutputLayers methods.

The stand-ins written here, and so the semantics that rest on them and not on the reference: `Boxes` (tensor, len, indexing, clip,
nonempty, cat), `Instances` (a bag of fields that does not check lengths), `Matcher` (Detectron2's rule: max over dim 0, thresholds
[-inf, t, inf] -> labels [0, 1], zeros for an empty matrix; it also records its outputs, which is where matched_idxs / matched_vals
come from), `pairwise_iou` (Detectron2's formula), `Box2BoxTransform` (apply_deltas / get_deltas with the scale clamp log(1000 / 16)),
fvcore's `smooth_l1_loss`, Detectron2's `cross_entropy` (F.cross_entropy, probabilities as targets included), `cat`, `nonzero_tuple`,
`_dense_box_regression_loss` (the smooth_l1 branch, for the hard-target case) and the event storage (put_scalar under name_scope).

One image has no ground truths.  The reference's _match_and_label_boxes leaves `gt_scores` unbound on that branch and assigns the
PREVIOUS image's tensor; the generator lets that run (the image is not the first) and then replaces the field by zeros, which is what
unmore_amd.box_loss.match_and_label documents.  Its rows are background, so no loss term reads those scores.

Batch: three images (4 ground truths of which two are the same box; none; one, a single-object image), 20 + 16 + 14 proposals, so
R % N != 0 and the reference's position-wise single-object indicator does not line up with the images.  Stored: the chain of three
stages (thresholds 0.5 / 0.6 / 0.7, weights (10,10,5,5) / (20,20,10,10) / (30,30,15,15), drop-loss on, soft targets) with proposals,
matches, predictions, drop weights, losses, gradients and logged scalars per stage; and on stage 0's inputs the variants drop-loss
off, hard targets with the drop weights, hard targets without.  float32 torch on the CPU.  Only arrays are stored."""
import contextlib
import math
import os
import sys
from typing import List, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from box_loss_common import STAGE_IOUS, STAGE_WEIGHTS  # noqa: E402

SIZES = [(48, 64), (40, 56), (52, 60)]
PROPOSALS = [20, 16, 14]
SINGLE = [0, 0, 1]
DROP_THRESH = 0.01
NUM_CLASSES = 1


# ---------------------------------------------------------------------------------------------------------------- stand-ins
class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor.reshape(-1, 4).to(torch.float32)

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, item):
        return Boxes(self.tensor[item].reshape(-1, 4))

    @property
    def device(self):
        return self.tensor.device

    def area(self):
        b = self.tensor
        return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])

    def clip(self, box_size):
        h, w = box_size
        x1, y1 = self.tensor[:, 0].clamp(min=0, max=w), self.tensor[:, 1].clamp(min=0, max=h)
        x2, y2 = self.tensor[:, 2].clamp(min=0, max=w), self.tensor[:, 3].clamp(min=0, max=h)
        self.tensor = torch.stack((x1, y1, x2, y2), dim=-1)

    def nonempty(self, threshold=0.0):
        b = self.tensor
        return ((b[:, 2] - b[:, 0]) > threshold) & ((b[:, 3] - b[:, 1]) > threshold)

    @classmethod
    def cat(cls, boxes_list):
        return cls(torch.cat([b.tensor for b in boxes_list], dim=0))


class Instances:
    def __init__(self, image_size, **fields):
        object.__setattr__(self, "_fields", dict(fields))
        object.__setattr__(self, "image_size", image_size)

    def __setattr__(self, name, value):
        self._fields[name] = value

    def __getattr__(self, name):
        fields = object.__getattribute__(self, "_fields")
        if name not in fields:
            raise AttributeError(name)
        return fields[name]

    def has(self, name):
        return name in self._fields

    def __len__(self):
        for v in self._fields.values():
            return len(v)
        return 0


def pairwise_iou(boxes1, boxes2):
    area1, area2 = boxes1.area(), boxes2.area()
    b1, b2 = boxes1.tensor, boxes2.tensor
    wh = torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])
    wh.clamp_(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


class Matcher:
    log = []

    def __init__(self, thresholds, labels, allow_low_quality_matches=False):
        assert not allow_low_quality_matches
        self.thresholds, self.labels = [-float("inf")] + list(thresholds) + [float("inf")], labels

    def __call__(self, m):
        if m.numel() == 0:
            matches = m.new_full((m.size(1),), 0, dtype=torch.int64)
            labels = m.new_full((m.size(1),), self.labels[0], dtype=torch.int8)
            Matcher.log.append((matches, m.new_zeros(m.size(1)), labels))
            return matches, labels
        vals, matches = m.max(dim=0)
        labels = matches.new_full(matches.size(), 1, dtype=torch.int8)
        for l, low, high in zip(self.labels, self.thresholds[:-1], self.thresholds[1:]):
            labels[(vals >= low) & (vals < high)] = l
        Matcher.log.append((matches, vals, labels))
        return matches, labels


class Box2BoxTransform:
    def __init__(self, weights, scale_clamp=math.log(1000.0 / 16)):
        self.weights, self.scale_clamp = weights, scale_clamp

    def get_deltas(self, src_boxes, target_boxes):
        sw, sh = src_boxes[:, 2] - src_boxes[:, 0], src_boxes[:, 3] - src_boxes[:, 1]
        scx, scy = src_boxes[:, 0] + 0.5 * sw, src_boxes[:, 1] + 0.5 * sh
        tw, th = target_boxes[:, 2] - target_boxes[:, 0], target_boxes[:, 3] - target_boxes[:, 1]
        tcx, tcy = target_boxes[:, 0] + 0.5 * tw, target_boxes[:, 1] + 0.5 * th
        wx, wy, ww, wh = self.weights
        deltas = torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), dim=1)
        assert (sw > 0).all().item(), "Input boxes to Box2BoxTransform are not valid!"
        return deltas

    def apply_deltas(self, deltas, boxes):
        deltas = deltas.float()
        boxes = boxes.to(deltas.dtype)
        w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
        wx, wy, ww, wh = self.weights
        dx, dy, dw, dh = deltas[:, 0::4] / wx, deltas[:, 1::4] / wy, deltas[:, 2::4] / ww, deltas[:, 3::4] / wh
        dw, dh = torch.clamp(dw, max=self.scale_clamp), torch.clamp(dh, max=self.scale_clamp)
        pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
        pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
        out = torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1)
        return out.reshape(deltas.shape)


def smooth_l1_loss(input, target, beta, reduction="none"):
    if beta < 1e-5:
        loss = torch.abs(input - target)
    else:
        n = torch.abs(input - target)
        loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    if reduction == "mean":
        return loss.mean() if loss.numel() > 0 else 0.0 * loss.sum()
    return loss.sum() if reduction == "sum" else loss


def cat(tensors, dim=0):
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim)


def cross_entropy(input, target, *, reduction="mean", **kwargs):
    if target.numel() == 0 and reduction == "mean":
        return input.sum() * 0.0
    return F.cross_entropy(input, target, reduction=reduction, **kwargs)


def nonzero_tuple(x):
    return x.nonzero().unbind(1)


def _dense_box_regression_loss(anchors, box2box_transform, pred_anchor_deltas, gt_boxes, fg_mask, box_reg_loss_type="smooth_l1",
                               smooth_l1_beta=0.0):
    assert box_reg_loss_type == "smooth_l1"
    anchors = cat(anchors)
    gt = torch.stack([box2box_transform.get_deltas(anchors, k) for k in gt_boxes])
    return smooth_l1_loss(cat(pred_anchor_deltas, dim=1)[fg_mask], gt[fg_mask], beta=smooth_l1_beta, reduction="sum")


class Storage:
    def __init__(self):
        self.scalars, self.prefix = {}, ""

    def put_scalar(self, name, value):
        self.scalars[self.prefix + name] = float(value)

    @contextlib.contextmanager
    def name_scope(self, name):
        old, self.prefix = self.prefix, name.rstrip("/") + "/"
        yield
        self.prefix = old


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---------------------------------------------------------------------------------------------------------------- the reference's lines
def cut(path, name, indent=""):
    """the source of `def name` at `indent` in `path`, decorators included, padded so that line numbers stay the file's"""
    with open(path) as f:
        lines = f.readlines()
    at = next(i for i, l in enumerate(lines) if l.startswith(f"{indent}def {name}("))
    start = at
    while lines[start - 1].startswith(indent + "@"):
        start -= 1
    end = at + 1
    while end < len(lines) and (not lines[end].strip() or lines[end].startswith(indent + " ") or lines[end].startswith(indent + ")")):
        end += 1
    body = "".join(l[len(indent):] if l.strip() else l for l in lines[start:end])
    return compile("\n" * start + body, path, "exec")


def load_reference(ref, storage):
    ns = {"torch": torch, "F": F, "List": List, "Tuple": Tuple, "Union": Union, "Boxes": Boxes, "Instances": Instances, "cat": cat,
          "cross_entropy": cross_entropy, "nonzero_tuple": nonzero_tuple, "smooth_l1_loss": smooth_l1_loss, "pairwise_iou": pairwise_iou,
          "Box2BoxTransform": Box2BoxTransform, "_dense_box_regression_loss": _dense_box_regression_loss,
          "get_event_storage": lambda: storage}
    path = os.path.join(ref, "cad", "structures", "boxes.py")
    with open(path) as f:
        exec(compile(f.read(), path, "exec"), ns)
    exec(cut(os.path.join(ref, "cad", "modeling", "box_regression.py"), "_soft_dense_box_regression_loss"), ns)
    fast = os.path.join(ref, "cad", "modeling", "roi_heads", "fast_rcnn.py")
    exec(cut(fast, "_log_classification_stats"), ns)
    for name in ("losses", "box_reg_loss", "predict_boxes"):
        exec(cut(fast, name, "    "), ns)
    cascade = os.path.join(ref, "cad", "modeling", "roi_heads", "custom_cascade_rcnn.py")
    for name in ("_forward_box", "_match_and_label_boxes", "_create_proposals_from_boxes"):
        exec(cut(cascade, name, "    "), ns)
    return ns


def bind(obj, ns, *names):
    for name in names:
        setattr(obj, name, ns[name].__get__(obj))


# ---------------------------------------------------------------------------------------------------------------- the batch
def make_batch(rng):
    gts = [np.array([[6, 5, 30, 28], [34, 10, 58, 40], [10, 30, 26, 44], [34, 10, 58, 40]], dtype=np.float32),      # 1 and 3: the same box
           np.zeros((0, 4), dtype=np.float32),
           np.array([[12, 14, 44, 46]], dtype=np.float32)]
    scores = [np.array([0.9, 0.35, 1.0, 0.6], dtype=np.float32), np.zeros(0, dtype=np.float32), np.array([0.75], dtype=np.float32)]
    props = []
    for (h, w), n, gt in zip(SIZES, PROPOSALS, gts):
        p = np.zeros((n, 4), dtype=np.float32)
        for j in range(n):
            if len(gt) and j % 3 != 2:
                g = gt[rng.randint(len(gt))]
                p[j] = g + rng.uniform(-0.2, 0.2, 4) * np.array([g[2] - g[0], g[3] - g[1]] * 2)
            else:
                x, y = rng.uniform(0, 0.7 * w), rng.uniform(0, 0.7 * h)
                p[j] = [x, y, x + rng.uniform(0.1, 0.3) * w, y + rng.uniform(0.1, 0.3) * h]
        if len(gt):
            p[0] = gt[-1]                                                       # an exact copy of a (duplicated) ground truth
        props.append(p)
    return gts, scores, props


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    storage = Storage()
    ns = load_reference(sys.argv[1], storage)
    rng = np.random.RandomState(31)
    gts, gt_scores, props = make_batch(rng)
    N = len(SIZES)
    arrays = {"n_images": np.int64(N), "sizes": np.array(SIZES, dtype=np.int64), "single": np.array(SINGLE, dtype=np.int64),
              "proposals_per_image": np.array(PROPOSALS, dtype=np.int64), "drop_thresh": np.float64(DROP_THRESH)}
    targets = []
    for k in range(N):
        arrays[f"im{k}_gt_boxes"], arrays[f"im{k}_gt_scores"] = gts[k], gt_scores[k]
        arrays[f"im{k}_gt_classes"] = np.zeros(len(gts[k]), dtype=np.int64)
        targets.append(Instances(SIZES[k], gt_boxes=Boxes(torch.from_numpy(gts[k])), gt_classes=torch.zeros(len(gts[k]), dtype=torch.int64),
                                 gt_scores=torch.from_numpy(gt_scores[k])))

    predictions, given_weights, stage_proposals = [], [], []

    def predictor(k, soft=True):
        p = Bag(num_classes=NUM_CLASSES, use_soft_targets=soft, use_sigmoid_ce=False, box2box_transform=Box2BoxTransform(STAGE_WEIGHTS[k]),
                smooth_l1_beta=0.0, box_reg_loss_type="smooth_l1", loss_weight={})
        bind(p, ns, "box_reg_loss", "predict_boxes")
        real = ns["losses"].__get__(p)

        def losses(preds, proposals, weights=None):
            given_weights.append(None if weights is None else weights.clone())
            stage_proposals.append(proposals)
            return real(preds, proposals, weights=weights)
        p.losses = losses
        p.real_losses = real
        return p

    def run_stage(features, proposals, k):
        R = sum(len(p) for p in proposals)
        scores = torch.from_numpy((rng.standard_normal((R, 2)) * 2).astype(np.float32)).requires_grad_(True)
        d = rng.standard_normal((R, 4)).astype(np.float32) * np.array(STAGE_WEIGHTS[k], dtype=np.float32) * 0.05
        d[1::9, 2] = 6.0 * STAGE_WEIGHTS[k][2]                                  # past the clamp: dw / ww = 6 > log(1000 / 16)
        d[4::11, 0] = 40.0 * STAGE_WEIGHTS[k][0]                                # 40 widths to the right: clips to zero width, dropped
        deltas = torch.from_numpy(d).requires_grad_(True)
        predictions.append((scores, deltas))
        return scores, deltas

    heads = Bag(box_in_features=[], num_cascade_stages=3, training=True, num_classes=NUM_CLASSES, use_droploss=True,
                droploss_iou_thresh=DROP_THRESH, box_predictor=[predictor(k) for k in range(3)],
                proposal_matchers=[Matcher([t], [0, 1], allow_low_quality_matches=False) for t in STAGE_IOUS], _run_stage=run_stage)
    bind(heads, ns, "_forward_box", "_create_proposals_from_boxes")
    real_match = ns["_match_and_label_boxes"].__get__(heads)

    def match(proposals, stage, tgts):
        out = real_match(proposals, stage, tgts)
        for p, t in zip(out, tgts):
            if len(t) == 0:
                p.gt_scores = torch.zeros(len(p.proposal_boxes))              # the reference left the previous image's tensor here
        return out
    heads._match_and_label_boxes = match

    first = [Instances(SIZES[k], proposal_boxes=Boxes(torch.from_numpy(props[k]))) for k in range(N)]
    first = heads._match_and_label_boxes(first, 0, targets)
    losses = heads._forward_box({}, first, targets, SINGLE)
    torch.stack(list(losses.values())).sum().backward()
    assert len(predictions) == 3 and len(Matcher.log) == 3 * N and len(given_weights) == 3
    for s in range(3):
        scores, deltas = predictions[s]
        props_s = stage_proposals[s]
        arrays[f"st{s}_scores"], arrays[f"st{s}_deltas"] = scores.detach().numpy(), deltas.detach().numpy()
        arrays[f"st{s}_grad_scores"], arrays[f"st{s}_grad_deltas"] = scores.grad.numpy(), deltas.grad.numpy()
        arrays[f"st{s}_weights"] = given_weights[s].numpy()
        arrays[f"st{s}_loss_cls"] = np.float32(losses[f"loss_cls_stage{s}"].item())
        arrays[f"st{s}_loss_box_reg"] = np.float32(losses[f"loss_box_reg_stage{s}"].item())
        sc = storage.scalars
        arrays[f"st{s}_num_fg_bg"] = np.array([sc[f"stage{s}/roi_head/num_fg_samples"], sc[f"stage{s}/roi_head/num_bg_samples"]])
        arrays[f"st{s}_scalars"] = np.array([sc.get(f"stage{s}/fast_rcnn/{n}", np.nan) for n in ("cls_accuracy", "fg_cls_accuracy", "false_negative")])
        for k in range(N):
            p = props_s[k]
            idx, vals, labels = Matcher.log[s * N + k]
            arrays[f"st{s}_im{k}_proposal_boxes"] = p.proposal_boxes.tensor.numpy()
            arrays[f"st{s}_im{k}_matched_idxs"], arrays[f"st{s}_im{k}_matched_vals"] = idx.numpy(), vals.numpy()
            arrays[f"st{s}_im{k}_labels"] = labels.numpy().astype(np.int64)
            arrays[f"st{s}_im{k}_gt_classes"], arrays[f"st{s}_im{k}_gt_boxes"] = p.gt_classes.numpy(), p.gt_boxes.tensor.numpy()
            arrays[f"st{s}_im{k}_gt_scores"] = p.gt_scores.numpy()
        print(f"stage {s}: R {scores.shape[0]}, loss_cls {arrays[f'st{s}_loss_cls']:.6f}, loss_box_reg {arrays[f'st{s}_loss_box_reg']:.6f}, "
              f"dropped {int((given_weights[s] == 0).sum())}, fg/bg {arrays[f'st{s}_num_fg_bg']}, scalars {arrays[f'st{s}_scalars']}")
    assert arrays["st1_scores"].shape[0] < arrays["st0_scores"].shape[0], "no box was dropped between the stages"
    assert arrays["st0_scores"].shape[0] % N != 0

    # the variants on stage 0's inputs, through FastRCNNOutputLayers.losses itself
    for name, soft, use_w in (("nodrop", True, False), ("hard_drop", False, True), ("hard_nodrop", False, False)):
        scores = predictions[0][0].detach().clone().requires_grad_(True)
        deltas = predictions[0][1].detach().clone().requires_grad_(True)
        out = predictor(0, soft).real_losses((scores, deltas), stage_proposals[0], weights=given_weights[0] if use_w else None)
        (out["loss_cls"] + out["loss_box_reg"]).backward()
        arrays[f"v_{name}_loss_cls"], arrays[f"v_{name}_loss_box_reg"] = np.float32(out["loss_cls"].item()), np.float32(out["loss_box_reg"].item())
        arrays[f"v_{name}_grad_scores"], arrays[f"v_{name}_grad_deltas"] = scores.grad.numpy(), deltas.grad.numpy()
        print(name, out["loss_cls"].item(), out["loss_box_reg"].item())
    path = os.path.join(HERE, "box_loss.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
