"""The NumPy restatement of the RPN's training half (tests/rpn_loss_common.py) pinned without a GPU -- a plain torch-CPU composition of
Detectron2's steps written here ([G, R] IoU matrix, max, the equality mask, subsample_labels driven by an imposed permutation,
F.binary_cross_entropy_with_logits, smooth-L1 with autograd gradients), pinned hash values, the hash's uniformity, the fixture cut from
the reference's own loss -- so that the GPU tests rest on something; and every host check of unmore_amd.rpn_loss that needs no device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_common as RC
import rpn_loss_common as C
from unmore_amd import _lib as L
from unmore_amd import rpn, rpn_loss

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the torch composition
def _torch_iou(gt, anchors):
    """Detectron2's pairwise_iou"""
    a1, a2 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    wh = (torch.min(gt[:, None, 2:], anchors[:, 2:]) - torch.max(gt[:, None, :2], anchors[:, :2])).clamp(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (a1[:, None] + a2 - inter), torch.zeros(1, dtype=inter.dtype))


def _torch_label_and_sample(anchors, gt, size, B, fraction, perm_pos, perm_neg, boundary=-1, lo=0.3, hi=0.7):
    """Matcher(thresholds, [0, -1, 1], allow_low_quality_matches=True) + the boundary filter + subsample_labels, whose two randperm
    draws are the given permutations of the positives and the negatives (in nonzero's order)"""
    R = anchors.shape[0]
    if gt.shape[0] == 0:
        idx, labels = torch.zeros(R, dtype=torch.int64), torch.zeros(R, dtype=torch.int8)
    else:
        m = _torch_iou(gt, anchors)
        vals, idx = m.max(dim=0)
        labels = torch.full((R,), 1, dtype=torch.int8)
        for l, a, b in ((0, -float("inf"), lo), (-1, lo, hi), (1, hi, float("inf"))):
            labels[(vals >= a) & (vals < b)] = l
        row_max, _ = m.max(dim=1)
        labels[(m == row_max[:, None]).nonzero()[:, 1]] = 1              # set_low_quality_matches_
    if boundary >= 0:
        h, w = size
        inside = (anchors[:, 0] >= -boundary) & (anchors[:, 1] >= -boundary) & (anchors[:, 2] < w + boundary) & (anchors[:, 3] < h + boundary)
        labels[~inside] = -1
    before = labels.clone()
    positive, negative = (labels == 1).nonzero().squeeze(1), (labels == 0).nonzero().squeeze(1)
    num_pos = min(positive.numel(), int(B * fraction))
    num_neg = min(negative.numel(), B - num_pos)
    pos_idx, neg_idx = positive[perm_pos[:num_pos]], negative[perm_neg[:num_neg]]
    labels.fill_(-1)
    labels[pos_idx], labels[neg_idx] = 1, 0
    return before, labels, idx


def _keys_of(perm, members, R):
    """keys that make `members[perm]` the descending-key order: the first of the permutation gets the largest key"""
    keys = np.zeros(R, np.int64)
    keys[np.asarray(members)[np.asarray(perm)]] = len(perm) - np.arange(len(perm))
    return keys


def test_labels_and_samples_equal_a_torch_composition():
    c = C.BASE
    cells, gts = C.base_cells(), C.base_gt()
    anchors = C.all_anchors(cells, c["strides"], c["maps"])
    ta = torch.from_numpy(anchors)
    assert np.array_equal(anchors, torch.cat(rpn.grid_anchors([torch.from_numpy(x) for x in cells], list(c["strides"]), list(c["maps"]))).numpy())
    rng = np.random.RandomState(5)
    for boundary in (-1, 0):
        plain = C.label_and_sample_np(cells, c["strides"], c["maps"], gts, c["image_sizes"], c["B"], c["fraction"], boundary=boundary)
        keys, perms = [], []
        for r in plain:
            pos, neg = np.nonzero(r["labels"] == 1)[0], np.nonzero(r["labels"] == 0)[0]
            pp, pn = rng.permutation(len(pos)), rng.permutation(len(neg))
            keys.append(_keys_of(pp, pos, len(anchors)) + _keys_of(pn, neg, len(anchors)))
            perms.append((pp, pn))
        ref = C.label_and_sample_np(cells, c["strides"], c["maps"], gts, c["image_sizes"], c["B"], c["fraction"], boundary=boundary, keys=keys)
        for n, r in enumerate(ref):
            before, after, idx = _torch_label_and_sample(ta, torch.from_numpy(gts[n]), c["image_sizes"][n], c["B"], c["fraction"],
                                                         torch.from_numpy(perms[n][0]), torch.from_numpy(perms[n][1]), boundary)
            assert np.array_equal(r["labels"], before.numpy()), (boundary, n)
            assert np.array_equal(r["dense"], after.numpy()), (boundary, n)
            assert np.array_equal(r["idx"], idx.numpy()), (boundary, n)
            if len(gts[n]):
                m = _torch_iou(torch.from_numpy(gts[n]), ta)
                assert np.array_equal(r["vals"].view(np.uint32), m.max(dim=0)[0].numpy().view(np.uint32))
                assert np.array_equal(r["row_max"].view(np.uint32), m.max(dim=1)[0].numpy().view(np.uint32))


def _torch_losses(logits, deltas, dense, matched, anchors, gts, B, weights, beta, lw, dtype):
    """RPN.losses: BCE with logits over the labels >= 0, smooth-L1 over the labels == 1 against get_deltas, both / (B N)"""
    N, A = logits[0].shape[:2]
    lg = [torch.tensor(x, dtype=dtype, requires_grad=True) for x in logits]
    dl = [torch.tensor(x, dtype=dtype, requires_grad=True) for x in deltas]
    flat_l = torch.cat([x.permute(0, 2, 3, 1).flatten(1) for x in lg], dim=1)
    flat_d = torch.cat([x.view(N, A, 4, x.shape[2], x.shape[3]).permute(0, 3, 4, 1, 2).flatten(1, -2) for x in dl], dim=1)
    labels = torch.from_numpy(np.stack(dense).astype(np.int64))
    valid, pos = labels >= 0, labels == 1
    an = torch.tensor(anchors, dtype=dtype)
    targets = []
    for n in range(N):
        g = torch.tensor(gts[n], dtype=dtype)[torch.from_numpy(matched[n])] if len(gts[n]) else torch.zeros((len(anchors), 4), dtype=dtype)
        g = torch.where(pos[n][:, None], g, an)                            # rows that are masked out: any finite box
        sw, sh = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
        scx, scy = an[:, 0] + 0.5 * sw, an[:, 1] + 0.5 * sh
        tw, th = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        tcx, tcy = g[:, 0] + 0.5 * tw, g[:, 1] + 0.5 * th
        wx, wy, ww, wh = weights
        targets.append(torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), dim=1))
    e = flat_d[pos] - torch.stack(targets)[pos]
    loc = e.abs().sum() if beta < 1e-5 else torch.where(e.abs() < beta, 0.5 * e ** 2 / beta, e.abs() - 0.5 * beta).sum()
    cls = F.binary_cross_entropy_with_logits(flat_l[valid], labels[valid].to(dtype), reduction="sum")
    cls, loc = cls * lw[0] / (B * N), loc * lw[1] / (B * N)
    (cls + loc).backward()
    return cls.item(), loc.item(), [x.grad.numpy() for x in lg], [x.grad.numpy() for x in dl]


@pytest.mark.parametrize("weights,beta,lw", [((1.0, 1.0, 1.0, 1.0), 0.0, (1.0, 1.0)), ((10.0, 10.0, 5.0, 5.0), 0.5, (2.0, 0.25))])
def test_losses_equal_a_torch_composition(weights, beta, lw):
    c = C.BASE
    cells, gts, ref = C.base_cells(), C.base_gt(), C.base_reference()
    logits, deltas = C.base_predictions()
    anchors = C.all_anchors(cells, c["strides"], c["maps"])
    samples = [(r["pos"], r["neg"], r["gt"]) for r in ref]
    want = _torch_losses(logits, deltas, [r["dense"] for r in ref], [r["idx"] for r in ref], anchors, gts, c["B"], weights, beta, lw,
                         torch.float64)
    got = C.losses_np(logits, deltas, samples, cells, c["strides"], gts, c["B"], weights, beta, lw)
    for k in (0, 1):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got[k], want[k])
    for g, w in zip(got[2] + got[3], want[2] + want[3]):
        assert np.array_equal(g != 0, w != 0)
        assert (np.abs(g - w) <= 1e-6 * np.abs(w)).all()


def test_the_localisation_sum_agrees_with_the_reference_fixture():
    fx = C.load_fixture()
    c = C.BASE
    # the fixture's inputs are the base case's samples ...
    ref = C.base_reference()
    anchors = C.all_anchors(C.base_cells(), c["strides"], c["maps"])
    idx = np.concatenate([np.concatenate([r["pos"], r["neg"]]) for r in ref])
    assert np.array_equal(fx["anchors"], anchors[idx])
    assert np.array_equal(fx["mask"], np.concatenate([np.arange(len(r["pos"]) + len(r["neg"])) < len(r["pos"]) for r in ref]))
    # ... and the restated terms on them give the reference's sums
    m = fx["mask"]
    for name, weights, beta in (("w1_b0", (1, 1, 1, 1), 0.0), ("w1_b05", (1, 1, 1, 1), 0.5), ("w10_b0", (10, 10, 5, 5), 0.0),
                                ("w10_b05", (10, 10, 5, 5), 0.5)):
        t = C.get_deltas_np(fx["anchors"][m], fx["gt_boxes"][m], weights)
        terms, _ = C.smooth_l1_np(fx["deltas"][m].astype(np.float64) - t, beta)
        assert abs(terms.sum() - float(fx[f"sum_{name}"])) <= 1e-6 * abs(terms.sum()), name
    # and losses_np itself on the base case
    logits, deltas = C.base_predictions()
    got = C.losses_np(logits, deltas, [(r["pos"], r["neg"], r["gt"]) for r in ref], C.base_cells(), c["strides"], C.base_gt(), c["B"])
    assert abs(got[4] - float(fx["sum_w1_b0"])) <= 1e-6 * abs(got[4])


# ---------------------------------------------------------------------------------------------------------------- the hash
def test_hash_pinned_values():
    # worked by hand from the written-out formula with Python integers
    def fmix(h):
        h ^= h >> 16
        h = h * 0x85ebca6b & 0xffffffff
        h ^= h >> 13
        h = h * 0xc2b2ae35 & 0xffffffff
        return h ^ (h >> 16)
    for seed, n, r in ((0, 0, 0), (1, 0, 0), (3, 2, 8960), ((1 << 40) + 5, 3, 123456), (-1, 1, 7)):
        s = seed & ((1 << 64) - 1)
        want = fmix(fmix(r ^ (s & 0xffffffff)) ^ ((n * 0x9e3779b9 + (s >> 32)) & 0xffffffff)) >> 1
        assert int(C.hash_keys(seed, n, r)) == want
    assert [int(C.hash_keys(s, n, r)) for s, n, r in ((0, 0, 0), (1, 0, 0), (3, 2, 8960), ((1 << 40) + 5, 3, 123456))] == \
        [0, 402107975, 798338869, 190414928]
    k = C.hash_keys(7, 1, np.arange(100000))
    assert k.min() >= 0 and k.max() < 1 << 31


def test_hash_samples_uniformly():
    pos = np.arange(40) * 7 + 3
    labels = np.full(400, -1, np.int8)
    labels[pos] = 1
    count = np.zeros(400, np.int64)
    for seed in range(2000):
        got, _, P, _ = C.sample_np(labels, C.hash_keys(seed, 0, np.arange(400)), 20, 0.5)
        assert P == 40 and len(got) == 10
        count[got] += 1
    sd = (2000 * 0.25 * 0.75) ** 0.5
    assert count.sum() == 20000 and (np.abs(count[pos] - 500) <= 5 * sd).all(), count[pos]


def test_sampling_ties_go_to_the_lower_index():
    labels = np.array([1, 0, 1, 1, 0, 0, 1, -1, 0, 1], np.int8)
    pos, neg, P, Q = C.sample_np(labels, np.zeros(10, np.int64), 6, 0.5)
    assert (P, Q) == (5, 4) and pos.tolist() == [0, 2, 3] and neg.tolist() == [1, 4, 5]
    pos, neg, _, _ = C.sample_np(labels, np.array([0, 9, 5, 0, 1, 9, 5, 9, 0, 7]), 6, 0.5)
    assert pos.tolist() == [2, 6, 9] and neg.tolist() == [1, 4, 5]
    pos, neg, _, _ = C.sample_np(labels, np.zeros(10, np.int64), 16, 0.25)       # both fall short of their shares
    assert pos.tolist() == [0, 2, 3, 6] and neg.tolist() == [1, 4, 5, 8]


# ---------------------------------------------------------------------------------------------------------------- the base case
def test_the_base_case_is_what_the_gpu_tests_need():
    c = C.BASE
    ref = C.base_reference()
    anchors = C.all_anchors(C.base_cells(), c["strides"], c["maps"])
    assert len(anchors) == 8961 and c["B"] == 64
    cap = int(c["B"] * c["fraction"])
    strong = [int((r["vals"] >= F32(0.7)).sum()) if r["usable"].any() else 0 for r in ref]
    P = [int(r["counters"][0]) for r in ref]
    assert P[0] > cap and ref[0]["counters"].tolist()[2:4] == [32, 32]
    assert 0 < P[1] < cap and ref[1]["counters"].tolist()[2:4] == [P[1], 64 - P[1]]      # its negatives fill the batch
    assert strong[0] > 0 and strong[1] > 0 and P[0] > strong[0] and P[1] > strong[1] and P[2] > strong[2]   # >= 0.7 and low-quality only
    gts = C.base_gt()
    ties = (C.iou_np(gts[0], anchors) == ref[0]["row_max"][:, None]).sum(axis=1)
    assert ties.max() >= 3                                                              # several anchors tied at one row maximum
    assert ref[3]["counters"].tolist() == [0, 8961, 0, 64, 0]                           # the empty image samples 64 negatives
    inside = C.base_reference(boundary=0)
    assert all(r["counters"][0] > 0 for r in inside[:3])
    assert all(r["counters"][1] < q["counters"][1] for r, q in zip(inside, ref))        # the filter removed anchors everywhere


def test_match_edges():
    cells = [RC.cell_anchors_np((32,), (1.0,))]
    anchors = C.all_anchors(cells, (16,), ((2, 2),))
    # a ground truth outside every anchor: row maximum 0, every anchor of IoU 0 with it -- all of them -- becomes 1, the index stays
    gt = np.array([[0, 0, 20, 20], [500, 500, 520, 520]], F32)
    m = C.match_np(gt, anchors)
    assert m["row_max"][1] == 0 and m["idx"].tolist() == [0, 0, 0, 0]
    assert C.label_np(m, gt, anchors, (64, 64)).tolist() == [1, 1, 1, 1]
    # without it: only the anchor that holds the row maximum
    m = C.match_np(gt[:1], anchors)
    # (anchor 3 = (0, 0, 32, 32) holds it: 400 / 1024 = 0.39, between the thresholds; anchor 1: 320 / 1104 = 0.29)
    assert C.label_np(m, gt[:1], anchors, (64, 64)).tolist() == [0, 0, 0, 1] and m["vals"][3] == F32(400) / F32(1024)
    assert C.label_np(m, gt[:1], anchors, (64, 64), allow_low_quality=False).tolist() == [0, 0, 0, -1]
    # a NaN ground truth takes no part and is counted
    bad = np.array([[np.nan, 0, 20, 20], [0, 0, 20, 20]], F32)
    mb = C.match_np(bad, anchors)
    assert mb["bad"] == 1 and mb["idx"].tolist() == [1, 1, 1, 1] and np.array_equal(mb["vals"], m["vals"]) and mb["row_max"][0] == 0
    assert C.label_np(mb, bad, anchors, (64, 64)).tolist() == [0, 0, 0, 1]
    # no ground truths: all 0; the boundary filter still applies
    m0 = C.match_np(np.zeros((0, 4), F32), anchors)
    assert C.label_np(m0, np.zeros((0, 4), F32), anchors, (64, 64)).tolist() == [0, 0, 0, 0]
    assert C.label_np(m0, np.zeros((0, 4), F32), anchors, (64, 64), boundary=16).tolist() == [0, 0, 0, 0]
    assert C.label_np(m0, np.zeros((0, 4), F32), anchors, (64, 64), boundary=0).tolist() == [-1, -1, -1, 0]


# ---------------------------------------------------------------------------------------------------------------- the host checks
def test_the_library_exports_the_entry_points():
    assert {"umr_rpn_label_sample", "umr_rpn_loss", "umr_rpn_loss_workspace"} <= set(L.exported_symbols())
    lib = L.lib()
    assert lib.umr_rpn_loss_workspace(4) == 4 * 24 and lib.umr_rpn_loss_workspace(0) == -1     # two float64 sums and a padded count per image


def _args():
    cells = rpn.cell_anchors([[32], [64]], [0.5, 1.0, 2.0])
    gts = [torch.zeros((2, 4)), torch.zeros((0, 4))]
    return cells, [4, 8], [(6, 8), (3, 4)], gts, [(24, 32), (24, 32)]


@pytest.mark.parametrize("kw,word", [
    ({"iou_thresholds": (0.3, 0.5, 0.7)}, "iou_thresholds"), ({"iou_labels": (0, 1, 1)}, "iou_labels"),
    ({"iou_thresholds": (0.7, 0.3)}, "ordered"), ({"batch_size_per_image": 1025}, "batch_size_per_image"),
    ({"batch_size_per_image": 0}, "batch_size_per_image"), ({"positive_fraction": 1.5}, "positive_fraction"),
    ({"seed": 1.5}, "seed"), ({"anchor_boundary_thresh": float("nan")}, "anchor_boundary_thresh"),
    ({"keys": torch.zeros((2, 5), dtype=torch.int32)}, "keys"), ({"keys": torch.zeros((2, 180), dtype=torch.int64)}, "keys"),
    ({"offset": 1.0}, "offset")])
def test_label_and_sample_refuses_before_any_launch(kw, word):
    cells, strides, maps, gts, sizes = _args()
    with pytest.raises(ValueError, match=word):
        rpn_loss.label_and_sample_anchors(cells, strides, maps, gts, sizes, **kw)


def test_label_and_sample_refuses_shapes_and_the_cpu():
    cells, strides, maps, gts, sizes = _args()
    with pytest.raises(ValueError, match="gt_boxes"):
        rpn_loss.label_and_sample_anchors(cells, strides, maps, gts[:1], sizes)
    with pytest.raises(ValueError, match="gt_boxes"):
        rpn_loss.label_and_sample_anchors(cells, strides, maps, [gts[0].double(), gts[1]], sizes)
    with pytest.raises(ValueError, match="feature sizes"):
        rpn_loss.label_and_sample_anchors(cells, strides, maps[:1], gts, sizes)
    with pytest.raises(ValueError, match="image_sizes"):
        rpn_loss.label_and_sample_anchors(cells, strides, maps, gts, [(24, 32), (24,)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rpn_loss.label_and_sample_anchors(cells, strides, maps, gts, sizes)


def test_rpn_losses_refuses_before_any_launch():
    cells, strides, maps, gts, sizes = _args()
    N, A, R = 2, 3, (6 * 8 + 3 * 4) * 3
    lg = [torch.zeros((N, A, h, w)) for h, w in maps]
    dl = [torch.zeros((N, 4 * A, h, w)) for h, w in maps]
    s = rpn_loss.AnchorSamples(torch.zeros((N, 256), dtype=torch.int32), torch.zeros((N, 256), dtype=torch.int32),
                               torch.zeros((N, 2), dtype=torch.int32), None, None, R, 256)
    with pytest.raises(ValueError, match="giou"):
        rpn_loss.rpn_losses(lg, dl, s, cells, strides, gts, box_reg_loss_type="giou")
    with pytest.raises(ValueError, match="samples"):
        rpn_loss.rpn_losses(lg, dl, None, cells, strides, gts)
    with pytest.raises(ValueError, match="batch"):
        rpn_loss.rpn_losses(lg, dl, s, cells, strides, gts, batch_size_per_image=128)
    with pytest.raises(ValueError, match="contiguous"):
        rpn_loss.rpn_losses([lg[0].transpose(2, 3).contiguous().transpose(2, 3), lg[1]], dl, s, cells, strides, gts)
    with pytest.raises(ValueError, match="one type"):
        rpn_loss.rpn_losses(lg, [dl[0].bfloat16(), dl[1]], s, cells, strides, gts)
    with pytest.raises(ValueError, match="expected"):
        rpn_loss.rpn_losses(lg, [dl[0][:, :8].contiguous(), dl[1]], s, cells, strides, gts)
    with pytest.raises(ValueError, match="smooth_l1_beta"):
        rpn_loss.rpn_losses(lg, dl, s, cells, strides, gts, smooth_l1_beta=-1.0)
    with pytest.raises(ValueError, match="box2box_weights"):
        rpn_loss.rpn_losses(lg, dl, s, cells, strides, gts, box2box_weights=(1, 1, 0, 1))
    with pytest.raises(ValueError, match="loss_weight"):
        rpn_loss.rpn_losses(lg, dl, s, cells, strides, gts, loss_weight={"loss_cls": 1.0})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rpn_loss.rpn_losses(lg, dl, s, cells, strides, gts)
