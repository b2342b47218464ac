"""What the ROI-head sampling tests share: a NumPy restatement of unmore_amd.roi_sample (Detectron2's ROIHeads.label_and_sample_proposals
as the module docstring specifies it), the seeded base batch that reaches every branch, the keys that impose a recorded order, and the
loader of tests/golden/roi_sample.npz.  Everything is float32 with one rounding per operation or an integer: the device must be EQUAL."""
import math
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_sample.npz")
SEED_SALT = 0x726f695f68656164
GT_LOGIT = F32(math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10))))
COUNTERS = ("positives", "negatives", "sampled_fg", "sampled_bg", "bad")
FIELDS = ("proposal_boxes", "objectness_logits", "gt_classes", "gt_boxes", "gt_scores", "matched_idxs", "sampled_idxs")


# ---------------------------------------------------------------------------------------------------------------- the steps
def iou_np(gt, boxes):
    """box_loss.hip's bl_iou: [G, 4], [R, 4] -> float32 [G, R]; 0 unless inter > 0; a NaN is handed on"""
    g, a = np.asarray(gt, F32).reshape(-1, 4), np.asarray(boxes, F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ga, aa = ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])).astype(F32), ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).astype(F32)
        w = (np.minimum(g[:, None, 2], a[None, :, 2]) - np.maximum(g[:, None, 0], a[None, :, 0])).astype(F32)
        h = (np.minimum(g[:, None, 3], a[None, :, 3]) - np.maximum(g[:, None, 1], a[None, :, 1])).astype(F32)
        w, h = np.where(w > 0, w, F32(0)), np.where(h > 0, h, F32(0))
        inter = (w * h).astype(F32)
        union = ((ga[:, None] + aa[None, :]).astype(F32) - inter).astype(F32)
        return np.where(inter > 0, inter / np.where(inter > 0, union, F32(1)), F32(0)).astype(F32)


def fmix32(h):
    """murmur3's 32-bit finaliser on uint32 values held in uint64 arrays"""
    h = np.asarray(h, np.uint64) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    return h


def hash_keys(seed, n, r):
    """the default key of candidate(s) r of image n: rpn_loss's hash of the salted seed, int64 in [0, 2^31)"""
    seed = (int(seed) & ((1 << 64) - 1)) ^ SEED_SALT
    lo, hi = seed & 0xffffffff, seed >> 32
    mix = (int(n) * 0x9e3779b9 + hi) & 0xffffffff
    r = np.asarray(r, np.uint64) & np.uint64(0xffffffff)
    return (fmix32(fmix32(r ^ np.uint64(lo)) ^ np.uint64(mix)) >> np.uint64(1)).astype(np.int64)


def match_np(cand, gt_boxes, gt_classes, threshold, num_classes):
    """step 2 of one image: matched index int64 [C], value float32 [C], foreground bool [C], class int64 [C], bad bool [C]"""
    cand, gt = np.asarray(cand, F32).reshape(-1, 4), np.asarray(gt_boxes, F32).reshape(-1, 4)
    C = len(cand)
    bad = ~np.isfinite(cand).all(axis=1)
    idx, val = np.zeros(C, np.int64), np.zeros(C, F32)
    if len(gt):
        iou = iou_np(gt, cand)
        m = np.where(np.isnan(iou), F32(-1), iou)                      # a NaN never wins the maximum
        idx, best = m.argmax(axis=0), m.max(axis=0)                    # argmax: the lowest index that attains it
        matched = (best >= 0) & ~bad
        idx, val = np.where(matched, idx, 0), np.where(matched, best, F32(0)).astype(F32)
        fg = matched & (best >= F32(threshold))
    else:
        fg = np.zeros(C, bool)
    cls = np.full(C, num_classes, np.int64)
    if len(gt):
        cls = np.where(fg, np.asarray(gt_classes, np.int64)[idx], num_classes)
    return idx, val, fg, cls, bad


def sample_np(cls, bad, keys, B, fraction, num_classes, order):
    """steps 3 - 5 of one image: (sampled r in row order, num_pos, num_neg, P, Q)"""
    keys = np.asarray(keys, np.int64) & 0x7fffffff
    keys = np.where(keys == 0, 1, keys)                                # the kernels keep 0 for "not in this pool"
    pos = np.nonzero((cls != -1) & (cls != num_classes) & ~bad)[0]
    neg = np.nonzero((cls == num_classes) & ~bad)[0]
    num_pos = min(len(pos), int(B * fraction))
    num_neg = min(len(neg), B - num_pos)

    def take(members, k):
        chosen = members[np.lexsort((members, -keys[members]))[:k]]    # the largest keys, equal keys to the lower r, in that order
        return chosen if order == "key" else np.sort(chosen)
    return np.concatenate([take(pos, num_pos), take(neg, num_neg)]).astype(np.int64), num_pos, num_neg, len(pos), len(neg)


def label_and_sample_np(proposals, targets, iou_threshold=0.5, num_classes=1, B=512, fraction=0.25, append_gt=True, seed=0, keys=None,
                        order="key"):
    """label_and_sample_proposals on the host.  proposals: per image (boxes [R, 4], logits [R]); targets: per image a dict with gt_boxes,
    gt_classes and optionally gt_scores.  Per image a dict of FIELDS (gt_scores when the targets have them), `counts` (num_pos, num_neg)
    and `counters` [5]"""
    out = []
    for n, ((boxes, logits), tg) in enumerate(zip(proposals, targets)):
        boxes, logits = np.asarray(boxes, F32).reshape(-1, 4), np.asarray(logits, F32).reshape(-1)
        gt, gc = np.asarray(tg["gt_boxes"], F32).reshape(-1, 4), np.asarray(tg["gt_classes"], np.int64).reshape(-1)
        cand, cl = boxes, logits
        if append_gt:
            cand, cl = np.concatenate([boxes, gt]), np.concatenate([logits, np.full(len(gt), GT_LOGIT, F32)])
        idx, val, fg, cls, bad = match_np(cand, gt, gc, iou_threshold, num_classes)
        k = hash_keys(seed, n, np.arange(len(cand))) if keys is None else np.asarray(keys[n])
        rows, num_pos, num_neg, P, Q = sample_np(cls, bad, k, B, fraction, num_classes, order)
        item = {"proposal_boxes": cand[rows], "objectness_logits": cl[rows], "gt_classes": cls[rows], "matched_idxs": idx[rows],
                "sampled_idxs": rows.astype(np.int32), "gt_boxes": gt[idx[rows]] if len(gt) else np.zeros((len(rows), 4), F32),
                "counts": (num_pos, num_neg), "counters": np.array([P, Q, num_pos, num_neg, int(bad.sum())], np.int64),
                "all_classes": cls, "all_vals": val, "all_idx": idx, "keys": k}
        if tg.get("gt_scores") is not None:
            gs = np.asarray(tg["gt_scores"], F32).reshape(-1)
            item["gt_scores"] = gs[idx[rows]] if len(gt) else np.zeros(len(rows), F32)
        out.append(item)
    return out


def keys_from_order(sampled, num_pos, C):
    """keys that make the recorded order the descending-key order: the j-th recorded positive gets 2^30 - j, every other candidate a key
    below all of those (1 .. 7 by index); the negatives likewise (the pools are disjoint, so they may share values)"""
    keys = 1 + np.arange(C, dtype=np.int64) % 7
    sampled = np.asarray(sampled, np.int64)
    keys[sampled[:num_pos]] = (1 << 30) - np.arange(num_pos)
    keys[sampled[num_pos:]] = (1 << 30) - np.arange(len(sampled) - num_pos)
    return keys


# ---------------------------------------------------------------------------------------------------------------- the base batch
BASE = {"B": 32, "fraction": 0.25, "threshold": 0.5, "num_classes": 1, "seed": 7, "frame": (64, 64),
        # (proposals, ground truths) per image: candidate counts 256, 255, 257 (the chunk edge), an image without ground truths, one
        # without proposals, one with fewer candidates than the batch, one with 257 ground truths (the tile edge)
        "RG": ((240, 16), (252, 3), (255, 2), (100, 0), (0, 6), (10, 2), (30, 257))}


def _boxes(rng, n, frame, lo=4.0, hi=24.0):
    h, w = frame
    bw, bh = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    x1, y1 = rng.uniform(0, 1, n) * (w - bw), rng.uniform(0, 1, n) * (h - bh)
    return np.stack([x1, y1, x1 + bw, y1 + bh], axis=1).astype(F32).reshape(-1, 4)


def base_batch(case=BASE):
    """(proposals [(boxes, logits)], targets [dict]) of the seeded base batch, NumPy arrays"""
    rng = np.random.RandomState(case["seed"])
    props, tgts = [], []
    for k, (R, G) in enumerate(case["RG"]):
        gt = _boxes(rng, G, case["frame"], 8.0, 30.0)
        p = _boxes(rng, R, case["frame"])
        if k in (0, 6) and G:                                           # two thirds of the proposals are jittered ground truths
            for j in range(0, R):
                if j % 3 != 2:
                    g = gt[rng.randint(G)]
                    p[j] = g + rng.uniform(-0.15, 0.15, 4).astype(F32) * np.array([g[2] - g[0], g[3] - g[1]] * 2, F32)
        if k == 0:
            gt[5] = gt[2]                                               # a duplicated ground truth: an IoU tie, the lower index wins
            p[1] = gt[2]
            gt[0] = [8, 8, 28, 28]
            p[0] = [8, 8, 28, 18]                                       # IoU with gt 0: 200 / 400 = 0.5, the threshold exactly
            p[7] = [np.nan, 4, 20, 20]                                  # a non-finite proposal
            p[8] = [4, 4, np.inf, 20]
        if k == 1:                                                      # small proposals away from the ground truths but for two
            p = _boxes(rng, R, case["frame"], 2.0, 5.0)
            p[3] = gt[1] + np.array([0.5, 0, 0.5, 0], F32)
            p[200] = gt[0]
        props.append((p, rng.standard_normal(R).astype(F32)))
        tgts.append({"gt_boxes": gt, "gt_classes": np.zeros(G, np.int64), "gt_scores": rng.uniform(0.1, 1.0, G).astype(F32)})
    return props, tgts


def base_keys(case=BASE, append_gt=True):
    """seeded keys of a few values, so that equal keys meet at the cut of a pool"""
    rng = np.random.RandomState(case["seed"] + 1)
    return [rng.randint(0, 4, R + (G if append_gt else 0)).astype(np.int64) for R, G in case["RG"]]


BIG = {"B": 512, "fraction": 0.25, "threshold": 0.5, "num_classes": 1, "seed": 11, "frame": (64, 64), "RG": ((2000, 20),)}


def big_batch():
    """one image at the recipe's batch of 512: 2 000 proposals and 20 ground truths, a third of the proposals near a ground truth"""
    rng = np.random.RandomState(BIG["seed"])
    (R, G), = BIG["RG"]
    gt, p = _boxes(rng, G, BIG["frame"], 8.0, 30.0), _boxes(rng, R, BIG["frame"])
    for j in range(0, R, 3):
        g = gt[rng.randint(G)]
        p[j] = g + rng.uniform(-0.15, 0.15, 4).astype(F32) * np.array([g[2] - g[0], g[3] - g[1]] * 2, F32)
    return [(p, rng.standard_normal(R).astype(F32))], [{"gt_boxes": gt, "gt_classes": np.zeros(G, np.int64),
                                                         "gt_scores": rng.uniform(0.1, 1.0, G).astype(F32)}]


HASH_SEEDS = range(64)


def hash_draw_batch():
    """one image with 40 positives (copies of one ground truth, jittered) among 100 proposals, no append: P = 40, cap 8"""
    rng = np.random.RandomState(3)
    gt = np.array([[10, 10, 50, 50]], F32)
    p = _boxes(rng, 100, (64, 64), 2.0, 6.0)
    p[:40] = gt[0] + rng.uniform(-2, 2, (40, 4)).astype(F32)
    return [(p, np.zeros(100, F32))], [{"gt_boxes": gt, "gt_classes": np.zeros(1, np.int64), "gt_scores": np.ones(1, F32)}]


_cache = {}


def reference(name, **kw):
    """the restatement of the base ("base") or big ("big") batch under the given arguments, computed once each and shared; read-only"""
    key = (name,) + tuple(sorted((k, str(v)) for k, v in kw.items()))
    if key not in _cache:
        case, (props, tgts) = (BASE, base_batch()) if name == "base" else (BIG, big_batch())
        args = {"iou_threshold": case["threshold"], "num_classes": case["num_classes"], "B": case["B"], "fraction": case["fraction"],
                "seed": case["seed"]}
        args.update(kw)
        if args.get("keys") == "base":
            args["keys"] = base_keys(append_gt=args.get("append_gt", True))
        _cache[key] = label_and_sample_np(props, tgts, **args)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------- the fixture
def load_fixture(path=GOLDEN):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def fixture_batch(fx):
    """(proposals, targets, keys from the recorded order) of the fixture"""
    props, tgts, keys = [], [], []
    for k in range(int(fx["n_images"])):
        props.append((fx[f"im{k}_proposal_boxes"], fx[f"im{k}_objectness_logits"]))
        tgts.append({"gt_boxes": fx[f"im{k}_gt_boxes"], "gt_classes": fx[f"im{k}_gt_classes"], "gt_scores": fx[f"im{k}_gt_scores"]})
        C = len(props[-1][0]) + len(tgts[-1]["gt_boxes"])
        keys.append(keys_from_order(fx[f"im{k}_sampled_idxs"], int(fx[f"im{k}_num_fg"]), C))
    return props, tgts, keys
