"""Generate tests/golden/rpn_loss.npz by running the REFERENCE's own dense box-regression loss on the base case's sampled anchors.

Run where the reference tree is at hand, never on the GPU box:
    python tests/golden/make_golden_rpn_loss.py /path/to/reference

What executes verbatim from the reference, read at generation time and compiled in a namespace of stand-ins; none of it is stored here:
  cad/modeling/box_regression.py                   _soft_dense_box_regression_loss
It is cut out from `def` to the end of its body because its file imports Detectron2 and fvcore, which are absent.  Detectron2's RPN
itself is not in the reference (cad/modeling/proposal_generator/__init__.py re-exports it), so labelling and sampling have no fixture:
tests/rpn_loss_common.py restates them from the specification and tests/test_rpn_loss_cpu.py ties them to a torch composition.

The stand-ins written here, and so the semantics that rest on them and not on the reference: `Boxes`, `cat`, `Box2BoxTransform.get_deltas`
(Detectron2's formula) and fvcore's `smooth_l1_loss`.

Inputs: the base case of tests/rpn_loss_common.py (its seeded ground truths, the hash keys of its seed, its seeded predictions): the
sampled anchors of all four images one after the other, positives and negatives, as ONE image of S anchors; fg_mask marks the positives;
fg_weights are ones; the matched ground truth of a negative is replaced by the unit box (its row is masked out).  The function runs as
the reference calls it (reduction="none") in float32 torch on the CPU, for smooth_l1_beta 0 and 0.5 and the box-to-box weights
(1, 1, 1, 1) and (10, 10, 5, 5).  Only arrays are stored: anchors, gt_boxes, deltas [S, 4], mask [S], and the four sums."""
import os
import sys
from typing import List, Union

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import rpn_common as RC  # noqa: E402
import rpn_loss_common as C  # noqa: E402

VARIANTS = (("w1_b0", (1.0, 1.0, 1.0, 1.0), 0.0), ("w1_b05", (1.0, 1.0, 1.0, 1.0), 0.5), ("w10_b0", (10.0, 10.0, 5.0, 5.0), 0.0),
            ("w10_b05", (10.0, 10.0, 5.0, 5.0), 0.5))


class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor

    @classmethod
    def cat(cls, boxes_list):
        return cls(torch.cat([b.tensor for b in boxes_list], dim=0))


class Box2BoxTransform:
    def __init__(self, weights):
        self.weights = weights

    def get_deltas(self, src_boxes, target_boxes):
        sw, sh = src_boxes[:, 2] - src_boxes[:, 0], src_boxes[:, 3] - src_boxes[:, 1]
        scx, scy = src_boxes[:, 0] + 0.5 * sw, src_boxes[:, 1] + 0.5 * sh
        tw, th = target_boxes[:, 2] - target_boxes[:, 0], target_boxes[:, 3] - target_boxes[:, 1]
        tcx, tcy = target_boxes[:, 0] + 0.5 * tw, target_boxes[:, 1] + 0.5 * th
        wx, wy, ww, wh = self.weights
        deltas = torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), dim=1)
        assert (sw > 0).all().item(), "Input boxes to Box2BoxTransform are not valid!"
        return deltas


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


def cut(path, name):
    """the source of the top-level `def name` in `path`, padded so that line numbers stay the file's"""
    with open(path) as f:
        lines = f.readlines()
    at = next(i for i, l in enumerate(lines) if l.startswith(f"def {name}("))
    end = at + 1
    while end < len(lines) and (not lines[end].strip() or lines[end].startswith(" ") or lines[end].startswith(")")):
        end += 1
    return compile("\n" * at + "".join(lines[at:end]), path, "exec")


def base_samples():
    """(anchors, matched gt boxes, deltas) [S, 4] float32 and the mask [S] of the base case's samples, image after image"""
    c = C.BASE
    cells, gts = C.base_cells(), C.base_gt()
    ref = C.base_reference()
    _, deltas = C.base_predictions()
    anchors = C.all_anchors(cells, c["strides"], c["maps"])
    a_rows, g_rows, d_rows, mask = [], [], [], []
    for n, r in enumerate(ref):
        idx = np.concatenate([r["pos"], r["neg"]])
        lv, a, pix = C.level_of(idx, c["maps"], c["A"])
        a_rows.append(anchors[idx])
        g = np.tile(np.array([[0, 0, 1, 1]], np.float32), (len(idx), 1))
        g[:len(r["pos"])] = gts[n][r["gt"][:len(r["pos"])]]
        g_rows.append(g)
        d_rows.append(np.stack([RC.gather_deltas(deltas[lv[j]][n], [pix[j] * c["A"] + a[j]], c["A"])[0] for j in range(len(idx))]))
        mask.append(np.arange(len(idx)) < len(r["pos"]))
    return np.concatenate(a_rows), np.concatenate(g_rows), np.concatenate(d_rows).astype(np.float32), np.concatenate(mask)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ns = {"torch": torch, "List": List, "Union": Union, "Boxes": Boxes, "Box2BoxTransform": Box2BoxTransform, "cat": cat,
          "smooth_l1_loss": smooth_l1_loss}
    exec(cut(os.path.join(sys.argv[1], "cad", "modeling", "box_regression.py"), "_soft_dense_box_regression_loss"), ns)
    fn = ns["_soft_dense_box_regression_loss"]
    anchors, gt, deltas, mask = base_samples()
    arrays = {"anchors": anchors, "gt_boxes": gt, "deltas": deltas, "mask": mask}
    fg = torch.from_numpy(mask).reshape(1, -1)
    for name, weights, beta in VARIANTS:
        out = fn([Boxes(torch.from_numpy(anchors))], Box2BoxTransform(weights), [torch.from_numpy(deltas).unsqueeze(0)], [torch.from_numpy(gt)],
                 torch.ones(int(mask.sum())), fg, "smooth_l1", beta, reduction="none")
        arrays[f"sum_{name}"] = np.float32(out.item())
        print(name, out.item())
    assert mask.sum() > 40 and (~mask).sum() > 100
    path = os.path.join(HERE, "rpn_loss.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
