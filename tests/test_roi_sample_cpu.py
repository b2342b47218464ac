"""The NumPy restatement of the ROI heads' proposal sampling (tests/roi_sample_common.py) pinned without a GPU -- the fixture recorded
from the reference's own label_and_sample_proposals, a plain torch-CPU composition of Detectron2's steps written here with its randperm
replaced by a given permutation, pinned values of the salted hash, the hash draw's uniformity -- so that the GPU tests rest on something;
the branches the seeded base batch must reach; and every host check of unmore_amd.roi_sample that needs no device."""
import numpy as np
import pytest
import torch

import roi_sample_common as C
import rpn_loss_common as RL
from unmore_amd import roi_sample

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the fixture
def test_restatement_equals_the_reference_fixture():
    fx = C.load_fixture()
    props, tgts, keys = C.fixture_batch(fx)
    ref = C.label_and_sample_np(props, tgts, float(fx["iou_threshold"]), int(fx["num_classes"]), int(fx["batch_size_per_image"]),
                                float(fx["positive_fraction"]), keys=keys, order="key")
    N = int(fx["n_images"])
    for k, r in enumerate(ref):
        assert np.array_equal(r["sampled_idxs"], fx[f"im{k}_sampled_idxs"]), k                  # the reference's rows, in its order
        assert r["counts"][0] == int(fx[f"im{k}_num_fg"]) and sum(r["counts"]) == len(fx[f"im{k}_sampled_idxs"]), k
        for name in ("proposal_boxes", "objectness_logits", "gt_boxes", "gt_scores"):
            assert np.array_equal(_bits(r[name]), _bits(fx[f"im{k}_out_{name}"])), (k, name)
        assert np.array_equal(r["gt_classes"], fx[f"im{k}_out_gt_classes"]), k
    assert [sum(r["counts"][0] for r in ref) / N, sum(r["counts"][1] for r in ref) / N] == fx["scalars"].tolist()
    assert len(fx["im1_gt_boxes"]) == 0 and not fx["im1_out_gt_boxes"].any()                    # the image without ground truths
    assert np.array_equal(_bits(ref[0]["objectness_logits"][ref[0]["sampled_idxs"] >= 40]),
                          _bits(np.full(int((ref[0]["sampled_idxs"] >= 40).sum()), C.GT_LOGIT)))


# ---------------------------------------------------------------------------------------------------------------- the torch composition
def _torch_iou(gt, boxes):
    """Detectron2's pairwise_iou"""
    a1, a2 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    wh = (torch.min(gt[:, None, 2:], boxes[:, 2:]) - torch.max(gt[:, None, :2], boxes[:, :2])).clamp(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (a1[:, None] + a2 - inter), torch.zeros(1, dtype=inter.dtype))


def _torch_label_and_sample(boxes, logits, gt, gt_classes, gt_scores, threshold, num_classes, B, fraction, append, perm_pos, perm_neg):
    """add_ground_truth_to_proposals + pairwise_iou + Matcher([t], [0, 1]) + _sample_proposals with subsample_labels' two randperm
    draws replaced by the given permutations (of the positives and the negatives in nonzero's order) + the gathers"""
    if append:
        boxes, logits = torch.cat([boxes, gt]), torch.cat([logits, torch.full((len(gt),), float(C.GT_LOGIT))])
    if len(gt):
        vals, idx = _torch_iou(gt, boxes).max(dim=0)
        labels = (vals >= threshold).to(torch.int8)
        classes = gt_classes[idx].clone()
        classes[labels == 0] = num_classes
    else:
        idx, classes = torch.zeros(len(boxes), dtype=torch.int64), torch.zeros(len(boxes), dtype=torch.int64) + num_classes
    positive = ((classes != -1) & (classes != num_classes)).nonzero().squeeze(1)
    negative = (classes == num_classes).nonzero().squeeze(1)
    num_pos = min(positive.numel(), int(B * fraction))
    num_neg = min(negative.numel(), B - num_pos)
    sampled = torch.cat([positive[perm_pos[:num_pos]], negative[perm_neg[:num_neg]]])
    out = {"sampled_idxs": sampled, "proposal_boxes": boxes[sampled], "objectness_logits": logits[sampled], "gt_classes": classes[sampled],
           "matched_idxs": idx[sampled]}
    if len(gt):
        out["gt_boxes"], out["gt_scores"] = gt[idx[sampled]], gt_scores[idx[sampled]]
    return out, positive, negative


def _finite_batch():
    """the base batch without its two non-finite proposals: Detectron2 has no rule for those"""
    props, tgts = C.base_batch()
    p = props[0][0].copy()
    p[7], p[8] = [4, 4, 20, 20], [4, 4, 30, 20]
    return [(p, props[0][1])] + props[1:], tgts


@pytest.mark.parametrize("append", [True, False])
def test_restatement_equals_a_torch_composition(append):
    c = C.BASE
    props, tgts = _finite_batch()
    rng = np.random.RandomState(5)
    plain = C.label_and_sample_np(props, tgts, c["threshold"], c["num_classes"], c["B"], c["fraction"], append_gt=append)
    perms, keys = [], []
    for r in plain:
        cls = r["all_classes"]
        pos, neg = np.nonzero(cls != c["num_classes"])[0], np.nonzero(cls == c["num_classes"])[0]
        pp, pn = rng.permutation(len(pos)), rng.permutation(len(neg))
        k = np.ones(len(cls), np.int64)
        k[pos[pp]], k[neg[pn]] = (1 << 30) - np.arange(len(pp)), (1 << 30) - np.arange(len(pn))
        perms.append((pp, pn))
        keys.append(k)
    ref = C.label_and_sample_np(props, tgts, c["threshold"], c["num_classes"], c["B"], c["fraction"], append_gt=append, keys=keys)
    for n, (r, (boxes, logits), tg) in enumerate(zip(ref, props, tgts)):
        got, positive, negative = _torch_label_and_sample(
            torch.from_numpy(boxes), torch.from_numpy(logits), torch.from_numpy(tg["gt_boxes"]), torch.from_numpy(tg["gt_classes"]),
            torch.from_numpy(tg["gt_scores"]), c["threshold"], c["num_classes"], c["B"], c["fraction"], append,
            torch.from_numpy(perms[n][0]), torch.from_numpy(perms[n][1]))
        assert r["counters"][:2].tolist() == [positive.numel(), negative.numel()], n
        for name, v in got.items():
            v = v.numpy()
            if v.dtype == F32:
                assert np.array_equal(_bits(r[name]), _bits(v)), (n, name)
            else:
                assert np.array_equal(r[name], v), (n, name)
        if not len(tg["gt_boxes"]):
            assert not r["gt_boxes"].any() and not r["gt_scores"].any() and not r["matched_idxs"].any()


def test_order_index_is_the_same_sample_in_ascending_r():
    for kw in ({}, {"keys": "base"}):
        by_key, by_index = C.reference("base", **kw), C.reference("base", order="index", **kw)
        for a, b in zip(by_key, by_index):
            p = a["counts"][0]
            assert a["counts"] == b["counts"]
            assert np.array_equal(np.sort(a["sampled_idxs"][:p]), b["sampled_idxs"][:p])
            assert np.array_equal(np.sort(a["sampled_idxs"][p:]), b["sampled_idxs"][p:])


# ---------------------------------------------------------------------------------------------------------------- the hash
def test_pinned_values_of_the_salted_hash():
    """written out by hand from the formula: fmix(fmix(r ^ lo) ^ (n * 0x9e3779b9 + hi)) >> 1 on seed ^ 0x726f695f68656164"""
    def fmix(h):
        h ^= h >> 16
        h = h * 0x85ebca6b & 0xffffffff
        h ^= h >> 13
        h = h * 0xc2b2ae35 & 0xffffffff
        return h ^ (h >> 16)

    def key(seed, n, r):
        s = (seed & ((1 << 64) - 1)) ^ 0x726f695f68656164
        return fmix(fmix((r ^ s) & 0xffffffff) ^ ((n * 0x9e3779b9 + (s >> 32)) & 0xffffffff)) >> 1
    for seed, n, r in ((0, 0, 0), (0, 0, 1), (0, 3, 2019), (7, 1, 255), (-1, 65534, 16383), ((1 << 63) + 12345, 2, 100)):
        assert int(C.hash_keys(seed, n, r)) == key(seed, n, r), (seed, n, r)
    assert [int(C.hash_keys(0, 0, r)) for r in range(3)] == [982581396, 1500586665, 1227314558]
    assert int(C.hash_keys(7, 1, 255)) == 232585269
    # the salt: the same seed gives the RPN sampler other keys, and the salted seed gives it these
    r = np.arange(64)
    assert not np.array_equal(C.hash_keys(7, 1, r), RL.hash_keys(7, 1, r))
    assert np.array_equal(C.hash_keys(7, 1, r), RL.hash_keys(7 ^ C.SEED_SALT, 1, r))
    assert roi_sample.SEED_SALT == C.SEED_SALT and F32(roi_sample.GT_LOGIT) == C.GT_LOGIT


def test_the_hash_draw_is_uniform_enough():
    """each of 40 positives is drawn 8 / 40 of the time: 12.8 of 64 seeds expected, standard deviation 3.2; [3, 25] is wider than three
    standard deviations on either side"""
    props, tgts = C.hash_draw_batch()
    times = np.zeros(100, np.int64)
    for seed in C.HASH_SEEDS:
        r, = C.label_and_sample_np(props, tgts, 0.5, 1, 32, 0.25, append_gt=False, seed=seed)
        assert r["counters"][:4].tolist() == [40, 60, 8, 24]
        times[r["sampled_idxs"][:8]] += 1
    assert times[40:].sum() == 0 and times[:40].sum() == 64 * 8
    assert times[:40].min() >= 3 and times[:40].max() <= 25, times[:40]


# ---------------------------------------------------------------------------------------------------------------- the base batch
def test_the_base_batch_reaches_every_branch():
    c = C.BASE
    cap = int(c["B"] * c["fraction"])
    props, tgts = C.base_batch()
    ref, keyed = C.reference("base"), C.reference("base", keys="base")
    P = [int(r["counters"][0]) for r in ref]
    cand = [len(p[0]) + len(t["gt_boxes"]) for p, t in zip(props, tgts)]
    assert cand[:3] == [256, 255, 257] and cand[4] == 6 and len(props[4][0]) == 0           # the chunk edge; only appended ground truths
    assert len(tgts[3]["gt_boxes"]) == 0 and P[3] == 0 and ref[3]["counts"] == (0, c["B"])  # no ground truth: all background
    assert len(tgts[6]["gt_boxes"]) == 257                                                  # the ground-truth tile edge
    assert ref[6]["all_idx"].max() == 256                                                   # ... and the last tile's one entry is matched
    assert P[0] > cap and ref[0]["counts"] == (cap, c["B"] - cap)
    assert 0 < P[1] < cap and ref[1]["counts"] == (P[1], c["B"] - P[1])
    assert ref[4]["counts"] == (6, 0) and ref[5]["counters"][1] < c["B"] - ref[5]["counts"][0] and sum(ref[5]["counts"]) < c["B"]
    # the duplicated ground truth: candidates that attain their maximum at both copies are matched to the lower index
    iou = C.iou_np(tgts[0]["gt_boxes"], np.concatenate([props[0][0], tgts[0]["gt_boxes"]]))
    tie = (iou[2] == iou[5]) & (iou[2] == np.nanmax(iou, axis=0)) & (iou[2] > 0)
    assert tie.sum() >= 3 and (ref[0]["all_idx"][tie] == 2).all()
    assert ref[0]["all_vals"][0] == F32(0.5) and ref[0]["all_classes"][0] == 0              # on the threshold exactly: foreground
    assert ref[0]["counters"][4] == 2 and not np.isin([7, 8], ref[0]["sampled_idxs"]).any() # the non-finite proposals
    # two equal keys inside a pool at the cut: the last key taken equals the first one left out, in both pools of image 0
    r = keyed[0]
    k, cls = np.where(r["keys"] & 0x7fffffff == 0, 1, r["keys"] & 0x7fffffff), r["all_classes"]
    for part, members in ((r["sampled_idxs"][:cap], np.nonzero(cls == 0)[0]), (r["sampled_idxs"][cap:], np.nonzero(cls == 1)[0])):
        members = members[~np.isin(members, [7, 8])]
        left = np.setdiff1d(members, part)
        assert k[part].min() == k[left].max() and part[k[part] == k[part].min()].max() < left[k[left] == k[left].max()].min()
    # the appended ground truths are candidates: without the append image 4 has none at all
    off = C.reference("base", append_gt=False)
    assert off[4]["counts"] == (0, 0) and [len(r["all_classes"]) for r in off[:3]] == [240, 252, 255]
    assert any((r["sampled_idxs"] >= len(p[0])).any() for r, p in zip(ref, props))


def test_the_big_case_fills_the_recipe_batch():
    r, = C.reference("big")
    assert len(r["all_classes"]) == 2020 and r["counters"][0] > 128 and r["counts"] == (128, 384)


# ---------------------------------------------------------------------------------------------------------------- host checks
def _cpu_batch(R=5, G=2, N=2):
    props = [{"proposal_boxes": torch.zeros((R, 4)), "objectness_logits": torch.zeros(R)} for _ in range(N)]
    tgts = [{"gt_boxes": torch.zeros((G, 4)), "gt_classes": torch.zeros(G, dtype=torch.int64), "gt_scores": torch.ones(G)} for _ in range(N)]
    return props, tgts


def test_argument_errors_are_raised_before_any_launch():
    props, tgts = _cpu_batch()
    with pytest.raises(ValueError, match="more than 16384 per image"):
        big = {"proposal_boxes": torch.zeros((16383, 4)), "objectness_logits": torch.zeros(16383)}
        roi_sample.label_and_sample_proposals([props[0], big], tgts)
    with pytest.raises(ValueError, match="batch_size_per_image"):
        roi_sample.label_and_sample_proposals(props, tgts, batch_size_per_image=1025)
    with pytest.raises(ValueError, match="batch_size_per_image"):
        roi_sample.label_and_sample_proposals(props, tgts, batch_size_per_image=0)
    with pytest.raises(ValueError, match="between 1 and 65535 images"):
        roi_sample.label_and_sample_proposals([], [])
    with pytest.raises(ValueError, match="between 1 and 65535 images"):
        roi_sample.label_and_sample_proposals([props[0]] * 65536, [tgts[0]] * 65536)
    with pytest.raises(ValueError, match="targets: one per image"):
        roi_sample.label_and_sample_proposals(props, tgts[:1])
    with pytest.raises(ValueError, match=r"proposals\[1\]: proposal_boxes must be float32"):
        roi_sample.label_and_sample_proposals([props[0], {**props[1], "proposal_boxes": torch.zeros((5, 4), dtype=torch.float64)}], tgts)
    with pytest.raises(ValueError, match=r"targets\[0\]: gt_boxes must be float32"):
        roi_sample.label_and_sample_proposals(props, [{**tgts[0], "gt_boxes": torch.zeros((2, 4), dtype=torch.float16)}, tgts[1]])
    with pytest.raises(ValueError, match=r"proposals\[0\]: objectness_logits"):
        roi_sample.label_and_sample_proposals([{**props[0], "objectness_logits": torch.zeros(4)}, props[1]], tgts)
    with pytest.raises(ValueError, match=r"targets\[1\]: gt_classes must be integer"):
        roi_sample.label_and_sample_proposals(props, [tgts[0], {**tgts[1], "gt_classes": torch.zeros(2)}])
    with pytest.raises(ValueError, match="gt_scores in every target or in none"):
        roi_sample.label_and_sample_proposals(props, [tgts[0], {k: v for k, v in tgts[1].items() if k != "gt_scores"}])
    with pytest.raises(ValueError, match="same device"):
        roi_sample.label_and_sample_proposals([props[0], {**props[1], "proposal_boxes": torch.zeros((5, 4), device="meta")}], tgts)
    with pytest.raises(ValueError, match="iou_threshold is NaN"):
        roi_sample.label_and_sample_proposals(props, tgts, iou_threshold=float("nan"))
    with pytest.raises(ValueError, match="positive_fraction"):
        roi_sample.label_and_sample_proposals(props, tgts, positive_fraction=1.5)
    with pytest.raises(ValueError, match="order"):
        roi_sample.label_and_sample_proposals(props, tgts, order="random")
    with pytest.raises(ValueError, match="seed"):
        roi_sample.label_and_sample_proposals(props, tgts, seed=0.5)
    with pytest.raises(ValueError, match="num_classes"):
        roi_sample.label_and_sample_proposals(props, tgts, num_classes=-1)
    with pytest.raises(ValueError, match=r"keys\[1\] must be int32 \[7\]"):
        roi_sample.label_and_sample_proposals(props, tgts, keys=[torch.zeros(7, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)])
    with pytest.raises(ValueError, match=r"keys as one tensor must be int32 \[10\]"):
        roi_sample.label_and_sample_proposals(props, tgts, keys=torch.zeros(14, dtype=torch.int32), proposal_append_gt=False)
    with pytest.raises(ValueError, match="foreground takes"):
        roi_sample.foreground([{}])


def test_off_the_gpu_there_is_no_fallback():
    props, tgts = _cpu_batch()
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        roi_sample.label_and_sample_proposals(props, tgts)


def test_add_ground_truth_to_proposals_is_the_append():
    props, tgts = C.base_batch()
    tp = [(torch.from_numpy(b), torch.from_numpy(l)) for b, l in props]
    tt = [{k: torch.from_numpy(v) for k, v in t.items()} for t in tgts]
    for (boxes, logits), (b, l), t in zip(roi_sample.add_ground_truth_to_proposals(tt, tp), props, tgts):
        assert np.array_equal(_bits(boxes.numpy()), _bits(np.concatenate([b, t["gt_boxes"]])))
        assert np.array_equal(_bits(logits.numpy()), _bits(np.concatenate([l, np.full(len(t["gt_boxes"]), C.GT_LOGIT, F32)])))
    assert _bits(C.GT_LOGIT) == _bits(F32(23.025850929840455))
