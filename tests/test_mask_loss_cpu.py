"""unmore_amd.mask_loss without a GPU: hand-worked targets through the NumPy restatement (tests/mask_loss_common.py), the restatement
against the fixture the reference's own mask_rcnn_loss_weighted wrote (tests/golden/make_golden_mask_loss.py), the C-ABI entries'
argument checks, and the argument errors of the Python entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mask_loss_common import (blob_masks, load_fixture, logged_scalars, loss_reference, mask_averages_np, mask_targets_np,
                              roi_align_average)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("umr_mask_loss_workspace", "umr_mask_targets", "umr_mask_loss")


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("M", (4, 7))
def test_hand_worked_targets(dtype, M):
    """Every value is dyadic (coordinates are multiples of 1/4, weights of 1/16, counts 1 or 4), so every arithmetic order agrees."""
    rng = np.random.RandomState(M)
    H, W = 3 * M + 5, 3 * M + 2
    mask = rng.rand(H, W) < 0.5
    y0, x0 = 3, 2
    # an integer-aligned M x M box: grid 1, one sample at each pixel centre's index -> the window itself
    got = mask_targets_np(mask[None], np.array([[x0, y0, x0 + M, y0 + M]], dtype=np.float32), None, M, dtype)[0]
    assert np.array_equal(got, mask[y0:y0 + M, x0:x0 + M])
    # 2M x 2M: grid 2, the four samples of a bin are the four pixels of its 2 x 2 block -> "at least 2 of each block"
    win = mask[y0:y0 + 2 * M, x0:x0 + 2 * M].reshape(M, 2, M, 2).sum((1, 3))
    avg = roi_align_average(mask, np.array([x0, y0, x0 + 2 * M, y0 + 2 * M], dtype=np.float32), M, dtype)
    assert np.array_equal(avg, win / 4.0)
    assert np.array_equal(avg >= 0.5, win >= 2)
    # wholly outside [-1, H] x [-1, W]; zero and negative width
    full = np.ones((1, H, W), dtype=bool)
    for box in ((W + 2, 0, W + 2 + M, M), (0, -M - 3, M, -3), (-3 * M, -3 * M, -M, -M), (4, 4, 4, 4 + M), (4 + M, 4, 4, 4 + M), (4, 9, 4 + M, 5)):
        assert not mask_targets_np(full, np.array([box], dtype=np.float32), None, M, dtype).any(), box
    # a 1 x 1 mask with a box around it: every tap clamps to the one pixel, samples inside [-1, 1] count 1, the others 0
    one = np.ones((1, 1, 1), dtype=bool)
    avg = mask_averages_np(one, np.array([[-0.5, -0.5, 1.5, 1.5]], dtype=np.float32), None, 2, dtype)[0][0]
    assert np.array_equal(avg, np.ones((2, 2)))                 # samples at -0.5 and 0.5 on both axes
    avg = mask_averages_np(one, np.array([[-3.5, -0.5, 12.5, 1.5]], dtype=np.float32), None, 2, dtype)[0][0]
    # x: grid 8, samples -3.5 ... 3.5 (bin 0: -0.5 and 0.5 lie inside [-1, 1]) and 4.5 ... 11.5 (bin 1: none); y: -0.5 and 0.5
    assert np.array_equal(avg, np.array([[0.25, 0.0], [0.25, 0.0]]))
    assert not mask_targets_np(np.zeros((1, 1, 1), dtype=bool), np.array([[-0.5, -0.5, 1.5, 1.5]], dtype=np.float32), None, 2, dtype).any()


def test_bad_proposals_get_empty_targets():
    masks = np.ones((2, 6, 6), dtype=bool)
    boxes = np.array([[0, 0, 6, 6], [0, 0, 6, 6], [0, np.nan, 6, 6], [0, 0, 1e9, 6], [0, 0, np.inf, 6], [0, 0, 6, 6]], dtype=np.float32)
    avg, bad = mask_averages_np(masks, boxes, np.array([0, 2, 0, 0, 1, -1]), 3, np.float32)
    assert bad.tolist() == [False, True, True, True, True, True]
    assert avg[0].min() == 1.0 and not avg[1:].any()


def test_restatement_reproduces_the_fixture():
    """Targets exactly; loss, logged scalars and gradient in float64 to 1e-6 relative (the fixture is float32 torch on the CPU)."""
    fx = load_fixture()
    side, targets = fx["side"], []
    assert [im["boxes"].shape[0] for im in fx["images"]].count(0) == 1 and len(fx["images"]) == 3
    for im in fx["images"]:
        targets.append(mask_targets_np(im["masks"], im["boxes"], im["mask_index"], side, np.float32))
        assert np.array_equal(targets[-1], mask_targets_np(im["masks"], im["boxes"], im["mask_index"], side, np.float64))
    targets = np.concatenate(targets)
    assert np.array_equal(targets, fx["targets"])
    classes = np.concatenate([im["gt_classes"] for im in fx["images"]])
    w = fx["weights"]
    assert (w == 0).any() and ((w != 0) & (w != 1)).any()
    assert {c["logits"].shape[1] for c in fx["cases"].values()} == {1, 3}
    for name, case in fx["cases"].items():
        loss, counters, grad = loss_reference(case["logits"], targets, classes, w if case["weighted"] else None)
        assert abs(loss - case["loss"]) <= 1e-6 * abs(case["loss"]), name
        s = logged_scalars(counters, targets.size)
        assert np.allclose([s["accuracy"], s["false_positive"], s["false_negative"]], case["scalars"], rtol=1e-6, atol=0), name
        assert np.abs(grad - case["grad"]).max() <= 1e-6 * np.abs(case["grad"]).max(), name
        if case["logits"].shape[1] == 3:
            other = np.ones_like(grad, dtype=bool)
            other[np.arange(len(classes)), classes] = False
            assert not case["grad"][other].any() and case["grad"][~other].any()


def test_new_exports_are_declared_bound_and_check_their_arguments():
    from unmore_amd import _lib
    with open(os.path.join(ROOT, "include", "umr.h")) as f:
        declared = set(re.findall(r"\b(umr_[a-z0-9_]+)\s*\(", f.read()))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None
    assert "csrc/mask_loss.hip" in open(os.path.join(ROOT, "include", "umr.h")).read()
    assert lib.umr_mask_loss_workspace(-1, 28) == -1 and lib.umr_mask_loss_workspace(3, -1) == -1 and lib.umr_mask_loss_workspace(3, 0) == -1
    assert lib.umr_mask_loss_workspace(0, 28) > 0 and lib.umr_mask_loss_workspace(1000, 28) >= 1000 * 4 * 24
    vp = ctypes.c_void_p
    for call in (lambda: lib.umr_mask_loss(None, 0, 3, 1, 28, 10, 10, None, _lib.F32, None, None, 3, None, None, None, None, None, 0, None),
                 lambda: lib.umr_mask_targets(None, 0, 3, 28, 10, 10, None, None),
                 lambda: lib.umr_mask_targets(vp(8), 1, 3, 0, 10, 10, vp(8), None),               # side 0
                 lambda: lib.umr_mask_targets(vp(8), 1, -1, 28, 10, 10, vp(8), None),              # negative R
                 lambda: lib.umr_mask_targets(vp(8), 1, 3, 28, 6000, 6000, vp(8), None),           # tables past the LDS
                 lambda: lib.umr_mask_loss(vp(8), 1, 3, 1, 28, 10, 10, vp(8), 7, None, None, 3, None, vp(8), vp(8), vp(8), vp(8), 4096, None),
                 lambda: lib.umr_mask_loss(vp(8), 1, 3, 1, 28, 10, 10, vp(8), _lib.F32, None, None, 3, None, vp(8), vp(8), vp(8), vp(8), 8, None),
                 lambda: lib.umr_mask_loss(vp(8), 1, 3, 2, 28, 10, 10, vp(8), _lib.F32, None, None, 3, None, vp(8), vp(8), vp(8), vp(8), 4096, None),
                 lambda: lib.umr_mask_loss(vp(8), 1, 3, 1, 28, 10, 10, vp(8), _lib.F32, None, None, 4, None, vp(8), vp(8), vp(8), vp(8), 4096, None)):
        assert call() == -1
        assert b"mask_loss" in lib.umr_last_error_string()


def _instances(H=12, W=16, G=2, n=3, dev="cpu"):
    rng = np.random.RandomState(H + W)
    return {"gt_masks": torch.from_numpy(blob_masks(rng, H, W, G)).to(dev), "proposal_boxes": torch.rand(n, 4).to(dev) * 8,
            "mask_index": torch.zeros(n, dtype=torch.int64).to(dev), "gt_classes": torch.zeros(n, dtype=torch.int64).to(dev)}


def test_argument_errors_before_any_launch():
    from unmore_amd.mask_loss import mask_rcnn_loss, mask_rcnn_loss_weighted, mask_targets
    inst = _instances()
    x = torch.zeros(3, 1, 7, 7)
    w = torch.ones(3)
    for fn in (lambda: mask_rcnn_loss_weighted(x, [inst], w), lambda: mask_rcnn_loss(x, [inst]),
               lambda: mask_rcnn_loss_weighted(torch.zeros(0, 1, 7, 7), [], torch.ones(0)),
               lambda: mask_targets(inst["gt_masks"], inst["proposal_boxes"], inst["mask_index"], 7)):
        with pytest.raises(RuntimeError, match="no CPU fallback.*mask_loss_common"):
            fn()
    for bad_x, what in ((torch.zeros(3, 1, 7, 8), "square"), (torch.zeros(3, 1, 7), "logits must be"), (torch.zeros(3, 1, 7, 7).double(), "logits must be"),
                        (torch.zeros(4, 1, 7, 7), "4 rows of logits for 3 proposals"), (torch.zeros(3, 1, 600, 600), "side")):
        with pytest.raises(ValueError, match=what):
            mask_rcnn_loss_weighted(bad_x, [inst], w)
    for key, val, what in (("gt_masks", inst["gt_masks"].float(), "masks must be"), ("gt_masks", inst["gt_masks"][0], "masks must be"),
                           ("proposal_boxes", inst["proposal_boxes"].double(), "boxes must be"),
                           ("proposal_boxes", inst["proposal_boxes"][:, :3], "boxes must be"), ("proposal_boxes", None, "needs gt_masks"),
                           ("mask_index", inst["mask_index"][:2], "mask_index must be"), ("mask_index", inst["mask_index"].float(), "mask_index must be"),
                           ("mask_index", None, "3 boxes for 2 masks"), ("gt_masks", inst["gt_masks"].to("meta"), "same device")):
        broken = dict(inst)
        broken[key] = val
        with pytest.raises(ValueError, match=what):
            mask_rcnn_loss_weighted(x, [broken], w)
    for bad_w, what in ((torch.ones(2), "weights must be"), (torch.ones(3).double(), "weights must be"), (torch.ones(3).to("meta"), "same device")):
        with pytest.raises(ValueError, match=what):
            mask_rcnn_loss_weighted(x, [inst], bad_w)
    # more than one channel needs classes
    x3 = torch.zeros(3, 3, 7, 7)
    for val in (None, inst["gt_classes"][:2], inst["gt_classes"].float()):
        broken = dict(inst)
        broken["gt_classes"] = val
        with pytest.raises(ValueError, match="gt_classes"):
            mask_rcnn_loss_weighted(x3, [broken], w)
    # a frame whose sample tables do not fit the LDS (a view: nothing of that size is allocated)
    big = dict(inst)
    big["gt_masks"] = torch.zeros(1, 1, 1, dtype=torch.bool).expand(2, 6000, 6000)
    with pytest.raises(ValueError, match="LDS"):
        mask_rcnn_loss_weighted(x, [big], w)
    with pytest.raises(ValueError, match="equal length"):
        mask_targets([inst["gt_masks"]], [inst["proposal_boxes"], inst["proposal_boxes"]])
    with pytest.raises(ValueError, match="side"):
        mask_targets(inst["gt_masks"], inst["proposal_boxes"], inst["mask_index"], 0)


def test_detectron2_style_instances_are_read():
    """An object with .gt_masks.tensor / .proposal_boxes.tensor / .gt_classes goes through the same checks as a dict."""
    from types import SimpleNamespace as NS
    from unmore_amd.mask_loss import mask_rcnn_loss_weighted
    inst = _instances(G=3)
    obj = NS(gt_masks=NS(tensor=inst["gt_masks"]), proposal_boxes=NS(tensor=inst["proposal_boxes"]), gt_classes=inst["gt_classes"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mask_rcnn_loss_weighted(torch.zeros(3, 2, 7, 7), [obj], weights=torch.ones(3), vis_period=20)    # the head's own call, :1191
    with pytest.raises(ValueError, match="4 rows of logits for 3 proposals"):
        mask_rcnn_loss_weighted(torch.zeros(4, 2, 7, 7), [obj], torch.ones(4))
