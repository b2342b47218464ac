"""Generate tests/golden/mask_loss.npz by running the REFERENCE's own mask_rcnn_loss_weighted on the CPU.

Run where the reference tree is at hand, never on the GPU box:
    python tests/golden/make_golden_mask_loss.py /path/to/reference

What executes verbatim from the reference: the function `mask_rcnn_loss_weighted` of cad/modeling/roi_heads/roi_heads.py (from its
decorator to the line before the next top-level `def`).  The file as a whole imports Detectron2, which is absent, so exactly those lines
are read at generation time and compiled in a namespace of stand-ins written here; none of them is stored in this file.  The stand-ins:
`cat` (torch.cat), `get_event_storage` (an object that records put_scalar), `List`, `Instances`, and -- the one that matters --
`BitMasks.crop_and_resize`: Detectron2 implements it with torchvision's ROIAlign, neither is installed, so it calls the NumPy
restatement tests/mask_loss_common.py::mask_targets_np (float32).  The fixture therefore pins the weights, the mean, the channel
choice, the three logged scalars and the autograd gradient to the reference; the ROIAlign rule itself rests on that restatement and on
the hand-worked cases of tests/test_mask_loss_cpu.py.

Three images, the middle one without proposals; the reference gathers full frames by the matcher's index first
(`gt_masks[matched_idxs]`), which is what the stand-in does with `mask_index`.  Cases: one channel (class-agnostic), three channels with
gt_classes, and one channel with weights of ones (= Detectron2's unweighted mask_rcnn_loss); the weights include 0 and values other
than 1.  float32 torch on the CPU.  Only arrays are stored."""
import os
import sys
from typing import List

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mask_loss_common import blob_masks, jittered_proposals, mask_targets_np  # noqa: E402

SIDE = 14
SIZES = [(40, 56), (33, 47), (37, 61)]
MASKS = [4, 2, 3]
PROPOSALS = [5, 0, 4]


class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor


class BitMasks:
    def __init__(self, tensor):
        self.tensor = tensor

    def crop_and_resize(self, boxes, mask_size):
        return torch.from_numpy(mask_targets_np(self.tensor.numpy(), boxes.numpy(), None, mask_size, np.float32))


class Instances:
    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __len__(self):
        return self.proposal_boxes.tensor.shape[0]


class Storage:
    iter = 0

    def __init__(self):
        self.scalars = {}

    def put_scalar(self, name, value):
        self.scalars[name] = float(value)


def load_reference(ref_root, storage):
    path = os.path.join(ref_root, "cad", "modeling", "roi_heads", "roi_heads.py")
    with open(path) as f:
        lines = f.readlines()
    at = next(i for i, l in enumerate(lines) if l.startswith("def mask_rcnn_loss_weighted"))
    start = at - 1 if lines[at - 1].startswith("@") else at
    end = next(i for i in range(at + 1, len(lines)) if lines[i].startswith("def ") or lines[i].startswith("class "))
    ns = {"torch": torch, "F": F, "List": List, "Instances": Instances, "cat": lambda xs, dim=0: torch.cat(xs, dim=dim),
          "get_event_storage": lambda: storage}
    exec(compile("\n" * start + "".join(lines[start:end]), path, "exec"), ns)
    return ns["mask_rcnn_loss_weighted"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    storage = Storage()
    ref_loss = load_reference(sys.argv[1], storage)
    rng = np.random.RandomState(20)
    arrays = {"n_images": np.int64(len(SIZES)), "side": np.int64(SIDE)}
    instances, targets = [], []
    for k, ((H, W), G, n) in enumerate(zip(SIZES, MASKS, PROPOSALS)):
        masks = blob_masks(rng, H, W, G)
        boxes, idx = jittered_proposals(rng, masks, n, jitter=0.3)
        classes = rng.randint(0, 3, size=n).astype(np.int64)
        arrays[f"im{k}_masks"], arrays[f"im{k}_boxes"], arrays[f"im{k}_mask_index"], arrays[f"im{k}_gt_classes"] = masks, boxes, idx, classes
        gathered = torch.from_numpy(masks)[torch.from_numpy(idx)]               # gt_masks[matched_idxs]
        instances.append(Instances(gt_masks=BitMasks(gathered), proposal_boxes=Boxes(torch.from_numpy(boxes)),
                                   gt_classes=torch.from_numpy(classes)))
        targets.append(mask_targets_np(masks, boxes, idx, SIDE, np.float32))
    R = sum(PROPOSALS)
    weights = rng.uniform(0.2, 1.0, size=R).astype(np.float32)
    weights[1], weights[6], weights[3] = 0.0, 1.0, 2.5
    arrays["weights"], arrays["targets"] = weights, np.concatenate(targets)
    assert arrays["targets"].any() and not arrays["targets"].all()
    for name, C, w in (("c1", 1, weights), ("c3", 3, weights), ("c1_unweighted", 1, np.ones(R, dtype=np.float32))):
        logits = torch.from_numpy((rng.standard_normal((R, C, SIDE, SIDE)) * 3).astype(np.float32)).requires_grad_(True)
        loss = ref_loss(logits, instances, torch.from_numpy(w))
        loss.backward()
        s = storage.scalars
        arrays[f"{name}_logits"], arrays[f"{name}_loss"], arrays[f"{name}_grad"] = logits.detach().numpy(), np.float32(loss.item()), logits.grad.numpy()
        arrays[f"{name}_scalars"] = np.array([s["mask_rcnn/accuracy"], s["mask_rcnn/false_positive"], s["mask_rcnn/false_negative"]])
        print(name, loss.item(), arrays[f"{name}_scalars"])
    empty = ref_loss(torch.zeros(0, 1, SIDE, SIDE, requires_grad=True), [instances[1]], torch.zeros(0))
    assert float(empty) == 0.0 and empty.requires_grad                          # `pred_mask_logits.sum() * 0`
    path = os.path.join(HERE, "mask_loss.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
