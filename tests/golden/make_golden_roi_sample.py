"""Generate tests/golden/roi_sample.npz by running the REFERENCE's own ROIHeads.label_and_sample_proposals on the CPU.

Run where the reference tree is at hand, never on the GPU box:
    python tests/golden/make_golden_roi_sample.py /path/to/reference

What executes verbatim from the reference, read at generation time and compiled in a namespace of stand-ins; none of it is stored here:
  cad/modeling/roi_heads/roi_heads.py    ROIHeads._sample_proposals and ROIHeads.label_and_sample_proposals
The two methods are cut out (from `def` to the next `def` of the class, decorators included) because their file imports Detectron2,
which is absent.  They run with a stand-in `self` that carries the recipe's settings scaled down (batch 16, fraction 0.25, one class,
append on) and the matcher.

The stand-ins written here, and so the semantics that rest on them and not on the reference: `Boxes` (tensor, len, indexing, cat),
`Instances` (fields of one length; has, set, get_fields, indexing by an index tensor, cat), `Matcher` (Detectron2's rule: max over dim 0,
thresholds [-inf, t, inf] -> labels [0, 1], zeros for an empty matrix), `pairwise_iou` (Detectron2's formula), `subsample_labels`
(Detectron2's: nonzero, the two counts, torch.randperm twice), `add_ground_truth_to_proposals` (Detectron2's: the ground-truth boxes
appended with the logit log((1 - 1e-10) / (1 - (1 - 1e-10)))), and the event storage (put_scalar).  _sample_proposals is wrapped to record
its sampled_idxs: they are in the reference's row order, the positives first as positive[randperm], then the negatives.

Batch: three images in 64 x 48 frames -- 40 proposals and 4 ground truths of which two are the same box (more positives than the cap
of 4); 20 proposals and no ground truth (the reference sets no gt_* field there: the fixture stores zeros, which is what
unmore_amd.roi_sample documents); 30 proposals and 2 ground truths.  Stored per image: the inputs, the recorded
sampled_idxs, the number of foreground rows, every output field; and the two logged scalars.  float32 torch on the CPU.  Only arrays."""
import math
import os
import sys
from typing import List, Tuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SIZE = (48, 64)
RG = [(40, 4), (20, 0), (30, 2)]
BATCH, FRACTION, THRESHOLD, NUM_CLASSES = 16, 0.25, 0.5, 1


# ---------------------------------------------------------------------------------------------------------------- stand-ins
class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor.reshape(-1, 4).to(torch.float32)

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, item):
        return Boxes(self.tensor[item].reshape(-1, 4))

    def area(self):
        b = self.tensor
        return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])

    @classmethod
    def cat(cls, boxes_list):
        return cls(torch.cat([b.tensor for b in boxes_list], dim=0))


class Instances:
    def __init__(self, image_size, **fields):
        object.__setattr__(self, "_fields", {})
        object.__setattr__(self, "image_size", image_size)
        for k, v in fields.items():
            self.set(k, v)

    def __setattr__(self, name, value):
        self.set(name, value)

    def __getattr__(self, name):
        fields = object.__getattribute__(self, "_fields")
        if name not in fields:
            raise AttributeError(name)
        return fields[name]

    def set(self, name, value):
        for v in self._fields.values():
            assert len(v) == len(value), f"{name}: {len(value)} values for {len(v)} instances"
        self._fields[name] = value

    def has(self, name):
        return name in self._fields

    def get_fields(self):
        return self._fields

    def __len__(self):
        for v in self._fields.values():
            return len(v)
        return 0

    def __getitem__(self, item):
        return Instances(self.image_size, **{k: v[item] for k, v in self._fields.items()})

    @staticmethod
    def cat(instance_lists):
        out = Instances(instance_lists[0].image_size)
        for k in instance_lists[0].get_fields():
            values = [i.get_fields()[k] for i in instance_lists]
            out.set(k, Boxes.cat(values) if isinstance(values[0], Boxes) else torch.cat(values, dim=0))
        return out


def pairwise_iou(boxes1, boxes2):
    area1, area2 = boxes1.area(), boxes2.area()
    b1, b2 = boxes1.tensor, boxes2.tensor
    wh = torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])
    wh.clamp_(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


class Matcher:
    def __init__(self, thresholds, labels, allow_low_quality_matches=False):
        assert not allow_low_quality_matches
        self.thresholds, self.labels = [-float("inf")] + list(thresholds) + [float("inf")], labels

    def __call__(self, m):
        if m.numel() == 0:
            return m.new_full((m.size(1),), 0, dtype=torch.int64), m.new_full((m.size(1),), self.labels[0], dtype=torch.int8)
        vals, matches = m.max(dim=0)
        labels = matches.new_full(matches.size(), 1, dtype=torch.int8)
        for l, low, high in zip(self.labels, self.thresholds[:-1], self.thresholds[1:]):
            labels[(vals >= low) & (vals < high)] = l
        return matches, labels


def subsample_labels(labels, num_samples, positive_fraction, bg_label):
    positive = ((labels != -1) & (labels != bg_label)).nonzero().unbind(1)[0]
    negative = (labels == bg_label).nonzero().unbind(1)[0]
    num_pos = min(positive.numel(), int(num_samples * positive_fraction))
    num_neg = min(negative.numel(), num_samples - num_pos)
    perm1 = torch.randperm(positive.numel())[:num_pos]
    perm2 = torch.randperm(negative.numel())[:num_neg]
    return positive[perm1], negative[perm2]


def add_ground_truth_to_proposals(targets, proposals):
    out = []
    for t, p in zip(targets, proposals):
        value = math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10)))
        gt = Instances(p.image_size, proposal_boxes=t.gt_boxes, objectness_logits=value * torch.ones(len(t.gt_boxes)))
        out.append(Instances.cat([p, gt]))
    return out


class Storage:
    def __init__(self):
        self.scalars = {}

    def put_scalar(self, name, value):
        self.scalars[name] = float(value)


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
    ns = {"torch": torch, "np": np, "List": List, "Tuple": Tuple, "Instances": Instances, "pairwise_iou": pairwise_iou,
          "subsample_labels": subsample_labels, "add_ground_truth_to_proposals": add_ground_truth_to_proposals,
          "get_event_storage": lambda: storage}
    path = os.path.join(ref, "cad", "modeling", "roi_heads", "roi_heads.py")
    for name in ("_sample_proposals", "label_and_sample_proposals"):
        exec(cut(path, name, "    "), ns)
    return ns


# ---------------------------------------------------------------------------------------------------------------- the batch
def make_batch(rng):
    h, w = SIZE
    gts = [np.array([[6, 5, 30, 28], [34, 10, 58, 40], [10, 30, 26, 44], [34, 10, 58, 40]], dtype=np.float32),      # 1 and 3: the same box
           np.zeros((0, 4), dtype=np.float32),
           np.array([[12, 14, 44, 46], [40, 4, 60, 20]], dtype=np.float32)]
    props = []
    for k, ((R, G), gt) in enumerate(zip(RG, gts)):
        p = np.zeros((R, 4), dtype=np.float32)
        for j in range(R):
            if G and (j % 2 == 0 if k == 0 else j % 10 == 0):
                g = gt[rng.randint(G)]
                p[j] = g + rng.uniform(-0.12, 0.12, 4) * np.array([g[2] - g[0], g[3] - g[1]] * 2)
            else:
                x, y = rng.uniform(0, 0.7 * w), rng.uniform(0, 0.7 * h)
                p[j] = [x, y, x + rng.uniform(0.1, 0.3) * w, y + rng.uniform(0.1, 0.3) * h]
        if G:
            p[0] = gt[-1]                                                       # an exact copy of a (duplicated) ground truth
        props.append(p)
    return gts, props


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    storage = Storage()
    ns = load_reference(sys.argv[1], storage)
    rng = np.random.RandomState(47)
    torch.manual_seed(47)
    gts, props = make_batch(rng)
    N = len(RG)
    arrays = {"n_images": np.int64(N), "batch_size_per_image": np.int64(BATCH), "positive_fraction": np.float64(FRACTION),
              "iou_threshold": np.float64(THRESHOLD), "num_classes": np.int64(NUM_CLASSES)}
    targets, proposals = [], []
    for k in range(N):
        R, G = RG[k]
        scores, logits = rng.uniform(0.1, 1.0, G).astype(np.float32), rng.standard_normal(R).astype(np.float32)
        arrays[f"im{k}_gt_boxes"], arrays[f"im{k}_gt_scores"], arrays[f"im{k}_gt_classes"] = gts[k], scores, np.zeros(G, dtype=np.int64)
        arrays[f"im{k}_proposal_boxes"], arrays[f"im{k}_objectness_logits"] = props[k], logits
        targets.append(Instances(SIZE, gt_boxes=Boxes(torch.from_numpy(gts[k])), gt_classes=torch.zeros(G, dtype=torch.int64),
                                 gt_scores=torch.from_numpy(scores)))
        proposals.append(Instances(SIZE, proposal_boxes=Boxes(torch.from_numpy(props[k])), objectness_logits=torch.from_numpy(logits)))

    heads = Bag(batch_size_per_image=BATCH, positive_fraction=FRACTION, num_classes=NUM_CLASSES, proposal_append_gt=True,
                proposal_matcher=Matcher([THRESHOLD], [0, 1], allow_low_quality_matches=False))
    real_sample = ns["_sample_proposals"].__get__(heads)
    recorded = []

    def sample(matched_idxs, matched_labels, gt_classes):
        sampled_idxs, classes = real_sample(matched_idxs, matched_labels, gt_classes)
        recorded.append(sampled_idxs.clone())
        return sampled_idxs, classes
    heads._sample_proposals = sample
    out = ns["label_and_sample_proposals"].__get__(heads)(proposals, targets)
    assert len(out) == len(recorded) == N
    for k, (p, idx) in enumerate(zip(out, recorded)):
        S = len(idx)
        classes = p.gt_classes.numpy()
        n_fg = int((classes != NUM_CLASSES).sum())
        assert (classes[:n_fg] != NUM_CLASSES).all() and (classes[n_fg:] == NUM_CLASSES).all()
        arrays[f"im{k}_sampled_idxs"], arrays[f"im{k}_num_fg"] = idx.numpy().astype(np.int64), np.int64(n_fg)
        arrays[f"im{k}_out_proposal_boxes"] = p.proposal_boxes.tensor.numpy()
        arrays[f"im{k}_out_objectness_logits"] = p.objectness_logits.numpy()
        arrays[f"im{k}_out_gt_classes"] = classes
        if p.has("gt_boxes"):
            arrays[f"im{k}_out_gt_boxes"], arrays[f"im{k}_out_gt_scores"] = p.gt_boxes.tensor.numpy(), p.gt_scores.numpy()
        else:                                                                   # the reference set no gt_* field: zeros, as documented
            assert RG[k][1] == 0
            arrays[f"im{k}_out_gt_boxes"], arrays[f"im{k}_out_gt_scores"] = np.zeros((S, 4), np.float32), np.zeros(S, np.float32)
        print(f"image {k}: {RG[k]} -> {S} samples, {n_fg} foreground, order {idx.tolist()}")
    arrays["scalars"] = np.array([storage.scalars["roi_head/num_fg_samples"], storage.scalars["roi_head/num_bg_samples"]])
    print("scalars", arrays["scalars"])
    path = os.path.join(HERE, "roi_sample.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
