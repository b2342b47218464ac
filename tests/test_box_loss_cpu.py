"""unmore_amd.box_loss without a GPU: the restatement (tests/box_loss_common.py) against the fixture the reference's own box branch wrote
(tests/golden/make_golden_box_loss.py), hand-worked cases through the restatement, the C-ABI entries' argument checks, and the argument
errors of the Python entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from box_loss_common import (SCALE_CLAMP, STAGE_IOUS, STAGE_WEIGHTS, apply_deltas_np, clip_np, distinct_rows, droploss_iou_max_np,
                             droploss_weights_np, get_deltas_np, load_fixture, logged_scalars, losses_reference, match_np, next_stage_np,
                             pairwise_iou_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("umr_box_loss_workspace", "umr_box_decode_workspace", "umr_box_match", "umr_box_decode", "umr_box_apply_deltas", "umr_box_get_deltas",
       "umr_box_drop_weights", "umr_box_loss")


def _stage(fx, s):
    N = int(fx["n_images"])
    ims = [{k: fx[f"st{s}_im{i}_{k}"] for k in ("proposal_boxes", "matched_idxs", "matched_vals", "labels", "gt_classes", "gt_boxes", "gt_scores")}
           for i in range(N)]
    flat = {k: np.concatenate([im[k] for im in ims]) for k in ("proposal_boxes", "gt_classes", "gt_boxes", "gt_scores")}
    return ims, flat


def test_restatement_reproduces_the_fixture():
    """Labels, indices, counts and IoUs equal; drop weights equal; losses and gradients in float64 to float32 rounding of the fixture's
    own float32 run (1e-6 relative: a mean of about 50 float32 terms)."""
    fx = load_fixture()
    N = int(fx["n_images"])
    sizes, single = [tuple(s) for s in fx["sizes"].tolist()], fx["single"].tolist()
    assert [len(fx[f"im{k}_gt_boxes"]) for k in range(N)] == [4, 0, 1] and single == [0, 0, 1]
    assert np.array_equal(fx["im0_gt_boxes"][1], fx["im0_gt_boxes"][3])                # the duplicated ground truth
    for s in range(3):
        ims, flat = _stage(fx, s)
        R = len(flat["proposal_boxes"])
        fg = bg = 0
        for k, im in enumerate(ims):
            m = match_np(im["proposal_boxes"], fx[f"im{k}_gt_boxes"], fx[f"im{k}_gt_classes"], fx[f"im{k}_gt_scores"], STAGE_IOUS[s])
            assert np.array_equal(m["matched_idxs"], im["matched_idxs"]), (s, k)
            assert np.array_equal(m["matched_vals"], im["matched_vals"]), (s, k)       # bit for bit: float32 against float32
            assert np.array_equal(m["labels"], im["labels"] == 1) and np.array_equal(m["gt_classes"], im["gt_classes"])
            assert np.array_equal(m["gt_boxes"], im["gt_boxes"]) and np.array_equal(m["gt_scores"], im["gt_scores"])
            fg, bg = fg + m["num_fg"], bg + m["num_bg"]
        assert np.allclose([fg / N, bg / N], fx[f"st{s}_num_fg_bg"], rtol=1e-12)
        if s == 0:
            tie = ims[0]["matched_idxs"][0]
            assert tie == 1 and ims[0]["matched_vals"][0] == 1.0                       # a copy of ground truths 1 and 3: the lower index
        # drop weights
        boxes, gtb = [im["proposal_boxes"] for im in ims], [im["gt_boxes"] for im in ims]
        iou_max = droploss_iou_max_np(fx[f"st{s}_deltas"], boxes, gtb, STAGE_WEIGHTS[s], np.float32)
        w = droploss_weights_np(iou_max, float(fx["drop_thresh"]), single, N)
        assert np.array_equal(w, fx[f"st{s}_weights"]), s
        assert (w == 0).any() and (w == 1).any()
        # losses
        lc, lb, gs, gd, counters = losses_reference(fx[f"st{s}_scores"], fx[f"st{s}_deltas"], flat["proposal_boxes"], flat["gt_boxes"],
                                                    flat["gt_classes"], flat["gt_scores"], w, STAGE_WEIGHTS[s])
        assert abs(lc - fx[f"st{s}_loss_cls"]) <= 1e-6 * max(1, abs(lc)) and abs(lb - fx[f"st{s}_loss_box_reg"]) <= 1e-6 * max(1, abs(lb)), s
        assert np.abs(gs - fx[f"st{s}_grad_scores"]).max() <= 1e-6 * np.abs(gs).max()
        assert np.abs(gd - fx[f"st{s}_grad_deltas"]).max() <= 1e-6 * np.abs(gd).max()
        assert counters[0] == R and counters[6] == 0
        sc = logged_scalars(counters)
        want = dict(zip(("cls_accuracy", "fg_cls_accuracy", "false_negative"), fx[f"st{s}_scalars"]))
        assert {k for k, v in want.items() if not np.isnan(v)} == set(sc)
        assert all(abs(sc[k] - want[k]) <= 1e-12 for k in sc)
        # the next stage's proposals
        if s < 2:
            clipped, keep, counts = next_stage_np(fx[f"st{s}_deltas"], boxes, STAGE_WEIGHTS[s], sizes, True, np.float32)
            nxt, _ = _stage(fx, s + 1)
            assert counts.tolist() == [len(im["proposal_boxes"]) for im in nxt] and not keep.all()
            at = 0
            for k in range(N):
                kk = keep[at:at + len(boxes[k])]
                assert np.allclose(clipped[k][kk], nxt[k]["proposal_boxes"], rtol=1e-6, atol=1e-5), (s, k)    # one expf apart at the most
                at += len(boxes[k])
    # the variants on stage 0's inputs
    ims, flat = _stage(fx, 0)
    for name, soft, w in (("nodrop", True, None), ("hard_drop", False, fx["st0_weights"]), ("hard_nodrop", False, None)):
        lc, lb, gs, gd, _ = losses_reference(fx["st0_scores"], fx["st0_deltas"], flat["proposal_boxes"], flat["gt_boxes"], flat["gt_classes"],
                                             flat["gt_scores"], w, STAGE_WEIGHTS[0], use_soft_targets=soft)
        assert abs(lc - fx[f"v_{name}_loss_cls"]) <= 1e-6 * max(1, abs(lc)) and abs(lb - fx[f"v_{name}_loss_box_reg"]) <= 1e-6 * max(1, abs(lb)), name
        assert np.abs(gs - fx[f"v_{name}_grad_scores"]).max() <= 1e-6 * np.abs(gs).max(), name
        assert np.abs(gd - fx[f"v_{name}_grad_deltas"]).max() <= 1e-6 * np.abs(gd).max(), name


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_hand_worked_matching(dtype):
    gt = np.array([[0, 0, 2, 2]], dtype=np.float32)
    # [0,0,2,2] against [0,0,2,1]: intersection 2, union 4 + 2 - 2 = 4 -> exactly 0.5, foreground at t = 0.5
    m = match_np(np.array([[0, 0, 2, 1]]), gt, [0], [0.7], 0.5, 1, dtype)
    assert m["matched_vals"][0] == 0.5 and m["labels"][0] and m["gt_classes"][0] == 0 and m["gt_scores"][0] == np.float32(0.7)
    assert not match_np(np.array([[0, 0, 2, 1]]), gt, [0], [0.7], 0.6, 1, dtype)["labels"][0]
    # touching boxes: an intersection of zero width -> 0, background, but the fields are still gathered
    m = match_np(np.array([[2, 0, 4, 2], [0, 2, 2, 4], [5, 5, 6, 6]]), gt, [0], [0.7], 0.5, 1, dtype)
    assert not m["matched_vals"].any() and not m["labels"].any() and m["gt_classes"].tolist() == [1, 1, 1]
    assert np.array_equal(m["gt_boxes"], np.repeat(gt, 3, axis=0)) and m["num_bg"] == 3
    # a tie goes to the lower index: ground truths 1 and 2 are the same box
    gts = np.array([[10, 10, 12, 12], [0, 0, 2, 2], [0, 0, 2, 2]], dtype=np.float32)
    m = match_np(np.array([[0, 0, 2, 2], [0, 0, 2, 1]]), gts, [0, 0, 0], [0.1, 0.2, 0.3], 0.5, 1, dtype)
    assert m["matched_idxs"].tolist() == [1, 1] and m["matched_vals"].tolist() == [1.0, 0.5] and m["gt_scores"].tolist() == [np.float32(0.2)] * 2
    # no ground truths: background, zero boxes and zero scores; a non-finite proposal: bad and background
    m = match_np(np.array([[0, 0, 2, 2]]), np.zeros((0, 4)), [], [], 0.5, 1, dtype)
    assert m["gt_classes"].tolist() == [1] and not m["gt_boxes"].any() and m["gt_scores"].tolist() == [0] and m["num_bg"] == 1
    m = match_np(np.array([[0, 0, 2, 2], [0, np.nan, 2, 2], [0, 0, np.inf, 2]]), gt, [0], [0.7], 0.5, 1, dtype)
    assert m["labels"].tolist() == [True, False, False] and m["bad"] == 2 and m["matched_vals"].tolist() == [1, 0, 0]
    # zero-area and negative-width boxes have no positive intersection
    assert not pairwise_iou_np(np.array([[1, 1, 1, 2], [2, 0, 0, 2]]), gt, dtype).any()


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_hand_worked_transforms(dtype):
    w = (10.0, 10.0, 5.0, 5.0)
    box = np.array([[10, 20, 30, 60]], dtype=np.float32)                              # 20 x 40, centre (20, 40)
    assert np.array_equal(apply_deltas_np(np.zeros((1, 4)), box, w, dtype), box)
    # dx = 5 / 10 = half a width to the right, dy = -2.5 / 10 = a quarter of a height up
    assert np.array_equal(apply_deltas_np(np.array([[5, -2.5, 0, 0]]), box, w, dtype), box + np.array([[10, -10, 10, -10]]))
    # the clamp at log(1000 / 16): dw / ww = 6 and 60 both give the width * 62.5 (to the rounding of exp)
    big, bigger = apply_deltas_np(np.array([[0, 0, 30, 0]]), box, w, dtype), apply_deltas_np(np.array([[0, 0, 300, 0]]), box, w, dtype)
    assert np.array_equal(big, bigger)
    assert abs((big[0, 2] - big[0, 0]) - 20 * 1000 / 16) <= 20 * 1000 / 16 * 4 * np.finfo(dtype).eps
    at = apply_deltas_np(np.array([[0, 0, 5 * SCALE_CLAMP * 0.999, 0]]), box, w, dtype)
    assert at[0, 2] - at[0, 0] < big[0, 2] - big[0, 0]                                # below the clamp it still grows
    # get_deltas inverts apply_deltas
    tgt = np.array([[12, 18, 36, 50]], dtype=np.float32)
    d = get_deltas_np(box, tgt, w, dtype)
    assert np.allclose(d, [[10 * 4 / 20, 10 * -6 / 40, 5 * np.log(24 / 20), 5 * np.log(32 / 40)]], rtol=1e-6)
    assert np.allclose(apply_deltas_np(d, box, w, dtype), tgt, rtol=1e-5)
    # a box that clips to zero width is dropped in training and kept at inference; order is preserved
    boxes = [np.array([[10, 10, 20, 20], [10, 10, 20, 20], [10, 10, 20, 20]], dtype=np.float32)]
    deltas = np.array([[0, 0, 0, 0], [100, 0, 0, 0], [1, 0, 0, 0]], dtype=np.float32)             # the middle one moves 10 widths right
    clipped, keep, counts = next_stage_np(deltas, boxes, w, [(30, 40)], True, dtype)
    assert keep.tolist() == [True, False, True] and counts.tolist() == [2] and clipped[0][1].tolist() == [40, 10, 40, 20]
    assert clipped[0][2].tolist() == [11, 10, 21, 20]
    _, keep, counts = next_stage_np(deltas, boxes, w, [(30, 40)], False, dtype)
    assert keep.all() and counts.tolist() == [3]
    assert clip_np(np.array([[-3, -4, 50, 60]]), (30, 40), dtype).tolist() == [[0, 0, 40, 30]]


def test_hand_worked_drop_weights():
    """The reference's quirks: the set is the first n rows with n the number of DISTINCT rows among the first 100; the single-object
    indicator goes by position r // (R // N)."""
    a, b = [0, 0, 4, 4], [10, 10, 14, 14]
    assert distinct_rows(np.array([a, a, b, a])) == 2 and distinct_rows(np.zeros((0, 4))) == 0
    assert distinct_rows(np.array([a] * 100 + [b])) == 1                               # only the first 100 rows are looked at
    # matched gt_boxes [a, a, b]: two distinct rows -> the set is rows 0 and 1 = {a, a}; a prediction on b finds nothing
    props = [np.array([a, a, b], dtype=np.float32)]
    iou = droploss_iou_max_np(np.zeros((3, 4)), props, [np.array([a, a, b], dtype=np.float32)], (10, 10, 5, 5))
    assert iou.tolist() == [1, 1, 0]
    assert droploss_weights_np(iou, 0.01, None, 1).tolist() == [1, 1, 0]
    assert droploss_weights_np(np.array([0.01, 0.0100001], dtype=np.float32), 0.01, None, 1).tolist() == [0, 1]     # <= thresh is dropped
    # R = 5, N = 2: R // N = 2 rows per position; rows 0-1 are "image 0", 2-3 "image 1", row 4 belongs to nobody
    z = np.zeros(5, dtype=np.float32)
    assert droploss_weights_np(z, 0.01, [0, 1], 2).tolist() == [0, 0, 1, 1, 0]
    assert droploss_weights_np(z, 0.01, [1, 0], 2).tolist() == [1, 1, 0, 0, 0]
    assert droploss_weights_np(z, 0.01, [1, 1, 1], 3).tolist() == [1, 1, 1, 0, 0]      # R // N = 1
    assert droploss_weights_np(np.zeros(2, dtype=np.float32), 0.01, [1, 1, 1], 3).tolist() == [0, 0]               # R // N = 0: nobody


def test_hand_worked_losses():
    """One foreground row with score 0.5 and one background row, logits of zero: CE = log 2 on both; L1 of the deltas times the score."""
    w4 = (10.0, 10.0, 5.0, 5.0)
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10]], dtype=np.float32)
    gtb = np.array([[1, 0, 11, 10], [0, 0, 0, 0]], dtype=np.float32)                   # target deltas (1, 0, 0, 0)
    lc, lb, gs, gd, counters = losses_reference(np.zeros((2, 2)), np.array([[3.0, 0, -2, 0], [9, 9, 9, 9]]), boxes, gtb, [0, 1], [0.5, 0.9],
                                                [1.0, 0.0], w4)
    assert abs(lc - np.log(2) / 2) < 1e-15                                            # the background row has weight 0
    assert abs(lb - (2 + 2) * 0.5 / 2) < 1e-15
    assert np.allclose(gs, [[0.5 * (0.5 - 0.5), 0.5 * (0.5 - 0.5)], [0, 0]]) and np.allclose(gd, [[0.25, 0, -0.25, 0], [0, 0, 0, 0]])
    assert counters == [2, 1, 1, 1, 0, 1, 0]                                          # argmax of a tie is column 0
    # beta = 1: 0.5 d^2 below it, |d| - 0.5 above it
    _, lb, _, gd, _ = losses_reference(np.zeros((2, 2)), np.array([[3.0, 0.5, 0, 0], [0, 0, 0, 0]]), boxes, gtb, [0, 1], [1, 1], None, w4,
                                       smooth_l1_beta=1.0)
    assert abs(lb - ((2 - 0.5) + 0.5 * 0.25 + 0 + 0) / 2) < 1e-15 and np.allclose(gd[0], [0.5, 0.25, 0, 0])
    # a foreground row with a non-positive extent adds nothing and is counted
    gtb[0] = [5, 0, 5, 10]
    _, lb, _, gd, counters = losses_reference(np.zeros((2, 2)), np.ones((2, 4)), boxes, gtb, [0, 1], [1, 1], None, w4)
    assert lb == 0 and not gd.any() and counters[6] == 1


def test_new_exports_are_declared_bound_and_check_their_arguments():
    from unmore_amd import _lib
    with open(os.path.join(ROOT, "include", "umr.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(umr_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None
    assert "csrc/box_loss.hip" in hdr and ctypes.sizeof(_lib.BlImage) == 56
    assert lib.umr_box_loss_workspace(-1) == -1 and lib.umr_box_loss_workspace(0) > 0 and lib.umr_box_loss_workspace(10) == 480
    assert lib.umr_box_decode_workspace(-1, 1) == -1 and lib.umr_box_decode_workspace(5, -1) == -1
    assert lib.umr_box_decode_workspace(300, 2) == 300 * 16 + 8
    vp, F32 = ctypes.c_void_p, _lib.F32
    p = vp(8)
    w = (10.0, 10.0, 5.0, 5.0)
    calls = (
        lambda: lib.umr_box_match(None, 0, 3, 1, 0.5, 1, p, p, p, p, p, p, None),                                  # a null table
        lambda: lib.umr_box_match(p, 1, -1, 0, 0.5, 1, p, p, p, p, p, p, None),                                    # negative R
        lambda: lib.umr_box_match(p, -1, 3, 1, 0.5, 1, p, p, p, p, p, p, None),
        lambda: lib.umr_box_match(p, 1, 300, 1, 0.5, 1, p, p, p, p, p, p, None),                                   # too few chunks
        lambda: lib.umr_box_match(p, 1, 3, 1, 0.5, 1, None, p, p, p, p, p, None),                                  # a null output
        lambda: lib.umr_box_match(p, 1, 3, 1, float("nan"), 1, p, p, p, p, p, p, None),
        lambda: lib.umr_box_decode(None, 0, 3, 1, p, F32, *w, 1, p, p, p, p, 4096, None),
        lambda: lib.umr_box_decode(p, 1, 3, 1, p, 7, *w, 1, p, p, p, p, 4096, None),                               # an unknown dtype
        lambda: lib.umr_box_decode(p, 1, 3, 1, p, F32, *w, 1, p, p, p, p, 8, None),                                # an undersized workspace
        lambda: lib.umr_box_decode(p, 1, 3, 1, p, F32, 0.0, 10.0, 5.0, 5.0, 1, p, p, p, p, 4096, None),            # a zero weight
        lambda: lib.umr_box_apply_deltas(p, 7, p, 3, *w, p, None),
        lambda: lib.umr_box_apply_deltas(p, F32, p, -3, *w, p, None),
        lambda: lib.umr_box_apply_deltas(None, F32, p, 3, *w, p, None),
        lambda: lib.umr_box_get_deltas(p, None, 3, *w, p, None),
        lambda: lib.umr_box_get_deltas(p, p, -1, *w, p, None),
        lambda: lib.umr_box_drop_weights(None, 0, 3, 1, p, F32, *w, 0.01, None, p, None),
        lambda: lib.umr_box_drop_weights(p, 1, 3, 1, p, 9, *w, 0.01, None, p, None),
        lambda: lib.umr_box_drop_weights(p, 1, 3, 1, p, F32, *w, 0.01, None, None, None),
        lambda: lib.umr_box_loss(None, 0, 3, 1, 2, 1, p, p, F32, *w, 0.0, 1, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),
        lambda: lib.umr_box_loss(p, 1, -3, 1, 2, 1, p, p, F32, *w, 0.0, 1, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),
        lambda: lib.umr_box_loss(p, 1, 3, 1, 2, 1, p, p, 7, *w, 0.0, 1, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),
        lambda: lib.umr_box_loss(p, 1, 3, 1, 2, 1, p, p, F32, *w, 0.0, 1, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 8, None),       # workspace
        lambda: lib.umr_box_loss(p, 1, 3, 1, 3, 2, p, p, F32, *w, 0.0, 1, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),    # soft, K1 3
        lambda: lib.umr_box_loss(p, 1, 3, 1, 3, 1, p, p, F32, *w, 0.0, 0, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),    # K1 != K + 1
        lambda: lib.umr_box_loss(p, 1, 3, 1, 2, 1, p, p, F32, *w, -1.0, 1, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),   # beta
        lambda: lib.umr_box_loss(p, 1, 3, 1, 2, 1, p, p, F32, *w, 0.0, 1, 1, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),    # no weights
        lambda: lib.umr_box_loss(p, 1, 3, 1, 2, 1, p, p, F32, *w, 0.0, 1, 3, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),    # drop_mode
        lambda: lib.umr_box_loss(p, 1, 3, 1, 2, 1, p, p, F32, *w, 0.0, 1, 0, 0.01, None, None, 4, p, p, p, p, p, p, p, 4096, None),    # phases
        lambda: lib.umr_box_loss(p, 1, 3, 1, 2, 1, None, p, F32, *w, 0.0, 1, 0, 0.01, None, None, 3, p, p, p, p, p, p, p, 4096, None),
    )
    for i, call in enumerate(calls):
        assert call() == -1, i
        assert b"box_loss" in lib.umr_last_error_string(), i


def _batch(dev="cpu"):
    g = torch.Generator().manual_seed(3)
    targets = [{"gt_boxes": torch.tensor([[0., 0, 8, 8], [4, 4, 12, 12]]), "gt_classes": torch.zeros(2, dtype=torch.int64), "gt_scores": torch.tensor([0.5, 1.0])},
               {"gt_boxes": torch.zeros(0, 4), "gt_classes": torch.zeros(0, dtype=torch.int64), "gt_scores": torch.zeros(0)}]
    props = [{"proposal_boxes": torch.rand(3, 4, generator=g) * 8}, {"proposal_boxes": torch.rand(2, 4, generator=g) * 8}]
    matched = [{"proposal_boxes": p["proposal_boxes"], "gt_boxes": torch.rand(len(p["proposal_boxes"]), 4, generator=g),
                "gt_classes": torch.zeros(len(p["proposal_boxes"]), dtype=torch.int64), "gt_scores": torch.rand(len(p["proposal_boxes"]), generator=g)}
               for p in props]
    return props, targets, matched


W4 = (10.0, 10.0, 5.0, 5.0)


def test_cpu_tensors_fail_loudly():
    from unmore_amd import box_loss as B
    props, targets, matched = _batch()
    scores, deltas = torch.zeros(5, 2), torch.zeros(5, 4)
    for fn in (lambda: B.match_and_label(props, targets, 0.5),
               lambda: B.next_stage_proposals(deltas, props, W4, [(10, 10), (10, 10)]),
               lambda: B.apply_deltas(deltas[:3], props[0]["proposal_boxes"], W4),
               lambda: B.get_deltas(props[0]["proposal_boxes"], props[0]["proposal_boxes"], W4),
               lambda: B.droploss_weights(deltas, matched, W4, 0.01, torch.zeros(2)),
               lambda: B.fast_rcnn_losses(scores, deltas, matched, box2box_weights=W4),
               lambda: B.fast_rcnn_losses(scores, deltas, matched, box2box_weights=W4, droploss=(0.01, None), stats={}),
               lambda: B.fast_rcnn_losses(torch.zeros(0, 2), torch.zeros(0, 4), [], box2box_weights=W4)):
        with pytest.raises(RuntimeError, match="no CPU fallback.*box_loss_common"):
            fn()


def test_argument_errors_before_any_launch():
    from types import SimpleNamespace as NS
    from unmore_amd import box_loss as B
    props, targets, matched = _batch()
    scores, deltas = torch.zeros(5, 2), torch.zeros(5, 4)
    # match_and_label
    for key, val, what in (("gt_boxes", targets[0]["gt_boxes"].double(), "gt_boxes must be"), ("gt_boxes", targets[0]["gt_boxes"][:, :3], "gt_boxes must be"),
                           ("gt_classes", torch.zeros(2), "gt_classes must be integer"), ("gt_classes", torch.zeros(3, dtype=torch.int64), "gt_classes must be"),
                           ("gt_scores", torch.zeros(2).double(), "gt_scores must be float32"), ("gt_scores", None, "gt_scores must be"),
                           ("gt_boxes", targets[0]["gt_boxes"].to("meta"), "same device")):
        broken = [dict(targets[0]), targets[1]]
        broken[0][key] = val
        with pytest.raises(ValueError, match=what):
            B.match_and_label(props, broken, 0.5)
    with pytest.raises(ValueError, match="proposal_boxes must be"):
        B.match_and_label([{"proposal_boxes": torch.zeros(3, 5)}, props[1]], targets, 0.5)
    with pytest.raises(ValueError, match="one target per image"):
        B.match_and_label(props, targets[:1], 0.5)
    with pytest.raises(ValueError, match="NaN"):
        B.match_and_label(props, targets, float("nan"))
    with pytest.raises(ValueError, match="num_classes"):
        B.match_and_label(props, targets, 0.5, -1)
    # an object with Detectron2's fields goes through the same checks as a dict
    obj = [NS(proposal_boxes=NS(tensor=p["proposal_boxes"])) for p in props]
    tobj = [NS(gt_boxes=NS(tensor=t["gt_boxes"]), gt_classes=t["gt_classes"], gt_scores=t["gt_scores"]) for t in targets]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.match_and_label(obj, tobj, 0.5)
    # next_stage_proposals and the transforms
    for args, what in (((deltas[:4], props, W4, [(10, 10), (10, 10)]), "4 rows of proposal_deltas for 5 proposals"),
                       ((deltas.double(), props, W4, [(10, 10), (10, 10)]), "proposal_deltas must be"),
                       ((torch.zeros(5, 8), props, W4, [(10, 10), (10, 10)]), "class-agnostic"),
                       ((deltas, props, (10, 10, 5), [(10, 10), (10, 10)]), "box2box_weights"),
                       ((deltas, props, (10, 10, 5, 0), [(10, 10), (10, 10)]), "box2box_weights"),
                       ((deltas, props, W4, [(10, 10)]), r"one finite, non-negative \(h, w\)"),
                       ((deltas, props, W4, [(10, 10), (10, float("nan"))]), r"one finite, non-negative \(h, w\)")):
        with pytest.raises(ValueError, match=what):
            B.next_stage_proposals(*args)
    with pytest.raises(ValueError, match="3 source boxes for 2 target boxes"):
        B.get_deltas(torch.zeros(3, 4), torch.zeros(2, 4), W4)
    with pytest.raises(ValueError, match="deltas must be"):
        B.apply_deltas(torch.zeros(3, 4, dtype=torch.float16), torch.zeros(3, 4), W4)
    # fast_rcnn_losses
    kw = dict(box2box_weights=W4)
    for args, extra, what in (((torch.zeros(5, 3), deltas, matched), {}, "3 columns of scores for 1 classes"),
                              ((torch.zeros(5, 3), deltas, matched), {"num_classes": 2}, r"soft targets need K \+ 1 == 2"),
                              ((scores.double(), deltas, matched), {}, "scores must be"),
                              ((torch.zeros(5), deltas, matched), {}, "scores must be"),
                              ((scores, deltas.bfloat16(), matched), {}, "scores are torch.float32 and proposal_deltas torch.bfloat16"),
                              ((torch.zeros(4, 2), deltas[:4], matched), {}, "4 rows of scores for 5 proposals"),
                              ((scores, deltas, matched), {"box_reg_loss_type": "giou"}, "only the smooth_l1"),
                              ((scores, deltas, matched), {"smooth_l1_beta": -1.0}, "smooth_l1_beta"),
                              ((scores, deltas, matched), {"num_classes": 0}, "num_classes"),
                              ((scores, deltas, matched), {"weights": torch.ones(4)}, "weights must be float32"),
                              ((scores, deltas, matched), {"weights": torch.ones(5).double()}, "weights must be float32"),
                              ((scores, deltas, matched), {"weights": torch.ones(5), "droploss": (0.01, None)}, "not both"),
                              ((scores, deltas, matched), {"droploss": 0.01}, "droploss must be"),
                              ((scores, deltas, matched), {"droploss": (0.01, torch.zeros(3))}, "is_single_object must be"),
                              ((scores, deltas, matched), {"droploss": (float("nan"), None)}, "NaN"),
                              ((scores, deltas, matched), {"weights": torch.ones(5).to("meta")}, "same device")):
        with pytest.raises(ValueError, match=what):
            B.fast_rcnn_losses(*args, **kw, **extra)
    for key, val, what in (("gt_boxes", matched[0]["gt_boxes"][:2], "2 matched gt_boxes for 3 proposals"), ("gt_classes", torch.zeros(3), "gt_classes must be integer"),
                           ("gt_scores", None, "gt_scores must be float32"), ("gt_boxes", None, "gt_boxes must be")):
        broken = [dict(matched[0]), matched[1]]
        broken[0][key] = val
        with pytest.raises(ValueError, match=what):
            B.fast_rcnn_losses(scores, deltas, broken, **kw)
    # hard targets need no gt_scores and take any K
    hard = [{k: v for k, v in m.items() if k != "gt_scores"} for m in matched]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.fast_rcnn_losses(torch.zeros(5, 4), deltas, hard, num_classes=3, use_soft_targets=False, **kw)
    with pytest.raises(ValueError, match="4 rows of proposal_deltas"):
        B.droploss_weights(deltas[:4], matched, W4, 0.01)
