"""What the RPN training-half tests share: a NumPy restatement of unmore_amd.rpn_loss (Detectron2's RPN.label_and_sample_anchors and
RPN.losses as the module docstring specifies them), step by step so that a test can enter it with the device's own intermediate
results, the base case and its seeded ground truths, and the loader of tests/golden/rpn_loss.npz.  Matching and labelling are float32
with one rounding per operation (what csrc/rpn_loss.hip writes out); the losses take a dtype and are the reference in float64."""
import os

import numpy as np

import rpn_common as RC

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpn_loss.npz")

# rpn_common.BASE's geometry with a fourth image: R = 8961 anchors per image, B = 64, G = (24, 6, 1, 0).  With seed 10 this generator
# gives positives (>= 0.7 + low-quality only) of 31 + 115, 7 + 15, 0 + 10 and 0: image 0 above the cap of 32, image 1 below it (seed 3
# puts 44 into image 1); tests/test_rpn_loss_cpu.py::test_the_base_case_is_what_the_gpu_tests_need checks the conditions.
BASE = {"N": 4, "A": 3, "strides": RC.BASE["strides"], "maps": RC.BASE["maps"], "sizes": RC.BASE["sizes"], "ratios": RC.BASE["ratios"],
        "image_sizes": ((160, 224), (150, 200), (97, 131), (97, 131)), "G": (24, 6, 1, 0), "B": 64, "fraction": 0.5, "seed": 10}
COUNTERS = ("positives", "negatives", "sampled_positives", "sampled_negatives", "bad")


# ---------------------------------------------------------------------------------------------------------------- anchors
def all_anchors(cells, strides, maps, offset=0.0):
    """the R anchors of an image, level after level: float32 [R, 4]"""
    return np.concatenate([RC.anchors_np(c, s, h, w, offset) for c, s, (h, w) in zip(cells, strides, maps)])


def level_of(r, maps, A):
    """global anchor indices -> (level, a, y * W + x)"""
    r = np.asarray(r, np.int64)
    first = np.concatenate([[0], np.cumsum([h * w * A for h, w in maps])])
    l = np.searchsorted(first, r, side="right") - 1
    f = r - first[l]
    return l, f % A, f // A


# ---------------------------------------------------------------------------------------------------------------- steps 1 - 3
def iou_np(gt, anchors, dtype=F32):
    """box_loss.hip's bl_iou: [G, 4], [R, 4] -> [G, R]; 0 unless inter > 0"""
    g, a = np.asarray(gt, dtype).reshape(-1, 4), np.asarray(anchors, dtype).reshape(-1, 4)
    ga, aa = ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])).astype(dtype), ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = (np.minimum(g[:, None, 2], a[None, :, 2]) - np.maximum(g[:, None, 0], a[None, :, 0])).astype(dtype)
        h = (np.minimum(g[:, None, 3], a[None, :, 3]) - np.maximum(g[:, None, 1], a[None, :, 1])).astype(dtype)
        w, h = np.where(w > 0, w, dtype(0)), np.where(h > 0, h, dtype(0))
        inter = (w * h).astype(dtype)
        union = ((ga[:, None] + aa[None, :]).astype(dtype) - inter).astype(dtype)
        return np.where(inter > 0, inter / np.where(inter > 0, union, dtype(1)), dtype(0)).astype(dtype)


def match_np(gt, anchors):
    """step 1's matching of one image: a dict of vals float32 [R], idx int64 [R], row_max float32 [G], usable bool [G], bad"""
    gt = np.asarray(gt, F32).reshape(-1, 4)
    R = len(anchors)
    usable = np.isfinite(gt).all(axis=1)
    vals, idx, row_max = np.zeros(R, F32), np.zeros(R, np.int64), np.zeros(len(gt), F32)
    if usable.any():
        iou = iou_np(gt[usable], anchors)
        where = np.nonzero(usable)[0]
        vals, idx = iou.max(axis=0), where[iou.argmax(axis=0)]           # argmax: the first index that reaches the maximum
        row_max[usable] = iou.max(axis=1)
    return {"vals": vals, "idx": idx, "row_max": row_max, "usable": usable, "bad": int((~usable).sum())}


def label_np(m, gt, anchors, image_size, thresholds=(0.3, 0.7), allow_low_quality=True, boundary=-1):
    """steps 1 - 3: the labels int8 [R] before sampling"""
    lo, hi = F32(thresholds[0]), F32(thresholds[1])
    v = m["vals"]
    labels = np.zeros(len(v), np.int8)
    if m["usable"].any():
        labels = np.where(v < lo, 0, np.where(v < hi, -1, 1)).astype(np.int8)
        if allow_low_quality:
            gt = np.asarray(gt, F32).reshape(-1, 4)[m["usable"]]
            iou = iou_np(gt, anchors)
            labels[(iou == m["row_max"][m["usable"]][:, None]).any(axis=0)] = 1
    if boundary >= 0:
        t, (h, w), a = F32(boundary), image_size, np.asarray(anchors, F32)
        inside = (a[:, 0] >= -t) & (a[:, 1] >= -t) & (a[:, 2] < F32(F32(w) + t)) & (a[:, 3] < F32(F32(h) + t))
        labels[~inside] = -1
    return labels


# ---------------------------------------------------------------------------------------------------------------- step 4
def fmix32(h):
    """murmur3's 32-bit finaliser on uint32 arrays"""
    h = np.asarray(h, np.uint64) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    return h


def hash_keys(seed, n, r):
    """the default key of anchor(s) r of image n: fmix(fmix(r ^ seed_lo) ^ (n * 0x9e3779b9 + seed_hi)) >> 1, int64 in [0, 2^31)"""
    seed = int(seed) & ((1 << 64) - 1)
    lo, hi = seed & 0xffffffff, seed >> 32
    mix = (int(n) * 0x9e3779b9 + hi) & 0xffffffff
    r = np.asarray(r, np.uint64) & np.uint64(0xffffffff)
    return (fmix32(fmix32(r ^ np.uint64(lo)) ^ np.uint64(mix)) >> np.uint64(1)).astype(np.int64)


def sample_np(labels, keys, B, fraction):
    """step 4 of one image: (positives ascending, negatives ascending, P, Q); the largest keys, equal keys to the lower r"""
    labels, keys = np.asarray(labels), np.asarray(keys, np.int64) & 0x7fffffff
    pos, neg = np.nonzero(labels == 1)[0], np.nonzero(labels == 0)[0]
    num_pos = min(len(pos), int(B * fraction))
    num_neg = min(len(neg), B - num_pos)

    def take(cand, k):
        order = np.lexsort((cand, -keys[cand]))
        return np.sort(cand[order[:k]])
    return take(pos, num_pos), take(neg, num_neg), len(pos), len(neg)


def label_and_sample_np(cells, strides, maps, gt_boxes, image_sizes, B, fraction, thresholds=(0.3, 0.7), allow_low_quality=True,
                        boundary=-1, offset=0.0, seed=0, keys=None):
    """label_and_sample_anchors on the host: per image a dict of vals, idx, row_max, labels (before sampling), pos, neg, gt (of pos then
    neg), counters [5], dense (labels after sampling)"""
    anchors = all_anchors(cells, strides, maps, offset)
    out = []
    for n, (gt, size) in enumerate(zip(gt_boxes, image_sizes)):
        m = match_np(gt, anchors)
        labels = label_np(m, gt, anchors, size, thresholds, allow_low_quality, boundary)
        k = hash_keys(seed, n, np.arange(len(anchors))) if keys is None else np.asarray(keys[n])
        pos, neg, P, Q = sample_np(labels, k, B, fraction)
        dense = np.full(len(anchors), -1, np.int8)
        dense[pos], dense[neg] = 1, 0
        out.append({**m, "labels": labels, "pos": pos, "neg": neg, "gt": m["idx"][np.concatenate([pos, neg])], "dense": dense,
                    "counters": np.array([P, Q, len(pos), len(neg), m["bad"]], np.int64)})
    return out


# ---------------------------------------------------------------------------------------------------------------- step 5
def get_deltas_np(src, target, weights, dtype=np.float64):
    """Box2BoxTransform.get_deltas in box_loss.hip's order"""
    s, t = np.asarray(src, dtype).reshape(-1, 4), np.asarray(target, dtype).reshape(-1, 4)
    wx, wy, ww, wh = (dtype(v) for v in weights)
    half = dtype(0.5)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sw, sh = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
        scx, scy = s[:, 0] + half * sw, s[:, 1] + half * sh
        tw, th = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
        tcx, tcy = t[:, 0] + half * tw, t[:, 1] + half * th
        return np.stack([wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * np.log(tw / sw), wh * np.log(th / sh)], axis=1).astype(dtype)


def smooth_l1_np(e, beta):
    """(terms, d terms / d e) of fvcore's smooth_l1_loss; beta < 1e-5: L1 with gradient 0 at 0"""
    a = np.abs(e)
    if beta < 1e-5:
        return a, np.sign(e)
    return np.where(a < beta, 0.5 * e * e / beta, a - 0.5 * beta), np.where(a < beta, e / beta, np.sign(e))


def losses_np(logits, deltas, samples, cells, strides, gt_boxes, B, weights=(1.0, 1.0, 1.0, 1.0), beta=0.0, loss_weight=(1.0, 1.0),
              offset=0.0, dtype=np.float64):
    """rpn_losses on the host.  logits[l] [N, A, H, W], deltas[l] [N, 4A, H, W] float arrays (bfloat16 inputs widened by the caller);
    samples: per image (pos, neg, gt of the positives).  Returns (loss_cls, loss_loc, grad logits per level, grad deltas per level,
    the sum of the smooth-L1 terms before the scale)."""
    N, A = logits[0].shape[:2]
    maps = [tuple(s.shape[2:]) for s in logits]
    anchors = all_anchors(cells, strides, maps, offset)
    g_l, g_d = [np.zeros(s.shape, dtype) for s in logits], [np.zeros(d.shape, dtype) for d in deltas]
    beta = float(F32(beta))
    sc, sl = dtype(loss_weight[0]) / dtype(B * N), dtype(loss_weight[1]) / dtype(B * N)
    cls_sum, loc_sum = dtype(0), dtype(0)
    for n, (pos, neg, gt_idx) in enumerate(samples):
        idx = np.concatenate([np.asarray(pos, np.int64), np.asarray(neg, np.int64)])
        t = np.concatenate([np.ones(len(pos), dtype), np.zeros(len(neg), dtype)])
        lv, a, pix = level_of(idx, maps, A)
        for j in range(len(idx)):
            flat = logits[lv[j]][n, a[j]].reshape(-1)
            x = dtype(flat[pix[j]])
            cls_sum += max(x, dtype(0)) - x * t[j] + np.log1p(np.exp(-abs(x)))
            with np.errstate(over="ignore"):
                g = dtype(1) / (dtype(1) + np.exp(-x)) - t[j]
            g_l[lv[j]][n, a[j]].reshape(-1)[pix[j]] = g * sc
        if len(pos):
            target = get_deltas_np(anchors[idx[:len(pos)]], np.asarray(gt_boxes[n], F32)[np.asarray(gt_idx, np.int64)[:len(pos)]], weights, dtype)
            for j in range(len(pos)):
                d = deltas[lv[j]][n].reshape(A, 4, -1)
                terms, grad = smooth_l1_np(d[a[j], :, pix[j]].astype(dtype) - target[j], beta)
                loc_sum += terms.sum()
                g_d[lv[j]][n].reshape(A, 4, -1)[a[j], :, pix[j]] = grad * sl
    return cls_sum * sc, loc_sum * sl, g_l, g_d, loc_sum


# ---------------------------------------------------------------------------------------------------------------- builders
def base_cells(case=BASE):
    return [RC.cell_anchors_np(s, case["ratios"]) for s in case["sizes"]]


def base_gt(case=BASE, seed=None):
    """per image G boxes: side log-uniform in [12, 0.9 min(h, w)], aspect log-uniform in [0.5, 2], placed uniformly inside the frame"""
    rng = np.random.RandomState(case["seed"] if seed is None else seed)
    out = []
    for (h, w), G in zip(case["image_sizes"], case["G"]):
        side = np.exp(rng.uniform(np.log(12.0), np.log(0.9 * min(h, w)), G))
        aspect = np.exp(rng.uniform(np.log(0.5), np.log(2.0), G))
        bw, bh = np.minimum(side / np.sqrt(aspect), w), np.minimum(side * np.sqrt(aspect), h)
        x1, y1 = rng.uniform(0, 1, G) * (w - bw), rng.uniform(0, 1, G) * (h - bh)
        out.append(np.stack([x1, y1, x1 + bw, y1 + bh], axis=1).astype(F32).reshape(-1, 4))
    return out


def base_predictions(case=BASE, seed=None):
    """seeded normal logits and normal * 0.2 deltas at the case's shapes: (logits, deltas) lists of float32 arrays"""
    return RC.base_inputs({**RC.BASE, "N": case["N"], "maps": case["maps"], "A": case["A"]}, case["seed"] + 100 if seed is None else seed)


_cache = {}


def base_reference(boundary=-1):
    """the restatement of the base case (hash keys, seed = the case's), computed once per boundary threshold and shared; read-only"""
    if boundary not in _cache:
        c = BASE
        _cache[boundary] = label_and_sample_np(base_cells(), c["strides"], c["maps"], base_gt(), c["image_sizes"], c["B"], c["fraction"],
                                               boundary=boundary, seed=c["seed"])
    return _cache[boundary]


def load_fixture(path=GOLDEN):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
