"""What the detector-inference tests share: a NumPy float32 restatement of unmore_amd.detector_inference (csrc/det_post.hip's written-out
operation order), a torch-CPU restatement of the paste that calls F.grid_sample exactly as Detectron2's _do_paste_mask does, seeded
input builders, the band rule and the fixture."""
import os

import numpy as np

from unmore_amd import rle

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
BAND = 1e-4            # a pixel may differ from float64 only where the float64 sample lies this close to the threshold (see band_check)
BAND_CAP = 1e-3        # and such pixels are at most this share of the pixels with a non-zero float64 value


# ---------------------------------------------------------------------------------------------------------------- selection
def clip_boxes(b, h, w):
    """Boxes.clip on float32 [n, 4] (a NaN stays a NaN)"""
    b = np.array(b, dtype=F32).reshape(-1, 4)
    hi = np.array([w, h, w, h], dtype=F32)
    out = b.copy()
    out[b < 0] = 0
    out = np.where(b > hi, hi, out)
    return out.astype(F32)


def iou_f32(a, b):
    """inter / ((area_a + area_b) - inter) in float32, every operation rounded on its own; 0 / 0 is NaN.  a: [4] or [4, n]; b: [4]"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    xx1, yy1 = np.maximum(a[0], b[0]), np.maximum(a[1], b[1])
    xx2, yy2 = np.minimum(a[2], b[2]), np.minimum(a[3], b[3])
    w, h = np.maximum(F32(0), (xx2 - xx1).astype(F32)), np.maximum(F32(0), (yy2 - yy1).astype(F32))
    inter = (w * h).astype(F32)
    area_a, area_b = ((a[2] - a[0]) * (a[3] - a[1])).astype(F32), ((b[2] - b[0]) * (b[3] - b[1])).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / ((area_a + area_b).astype(F32) - inter).astype(F32)).astype(F32)


def select_numpy(boxes, scores, shape, score_thresh, nms_thresh, topk):
    """fast_rcnn_inference_single_image: (boxes [n, 4] f32, scores [n] f32, classes [n] i64, rows [n] i64)"""
    boxes, scores = np.asarray(boxes, F32), np.asarray(scores, F32)
    R, K = scores.shape[0], scores.shape[1] - 1
    BC = boxes.shape[1] // 4
    valid = np.isfinite(boxes).all(axis=1) & np.isfinite(scores).all(axis=1)
    st, nt = F32(score_thresh), F32(nms_thresh)
    cand = [(r, c) for r in range(R) if valid[r] for c in range(K) if scores[r, c] > st]
    h, w = shape
    cb = [clip_boxes(boxes[r, (0 if BC == 1 else 4 * c):(0 if BC == 1 else 4 * c) + 4], h, w)[0] for r, c in cand]
    cs = np.array([scores[r, c] for r, c in cand], dtype=F32)
    order = np.argsort(-cs, kind="stable") if len(cand) else np.zeros(0, np.int64)       # descending, equal scores in candidate order
    kept, per_class = [], {}
    for i in order:
        if topk >= 0 and len(kept) >= topk:
            break
        mine = per_class.setdefault(cand[i][1], [])                            # the kept candidates of this class, earlier in the order
        with np.errstate(invalid="ignore"):
            if mine and (iou_f32(np.array([cb[j] for j in mine], dtype=F32).T, cb[i]) > nt).any():
                continue
        kept.append(i)
        mine.append(i)
    return (np.array([cb[i] for i in kept], dtype=F32).reshape(-1, 4), cs[kept].astype(F32),
            np.array([cand[i][1] for i in kept], dtype=np.int64), np.array([cand[i][0] for i in kept], dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------- the paste
def sigmoid_f32(x):
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x, dtype=F32))).astype(F32)


def _axis(n, lo, hi, M):
    """the pixel centres i + 0.5, i in [0, n), against the box side [lo, hi]: (floor index, weight of it, weight of the next), float32"""
    i = np.arange(n, dtype=F32)
    with np.errstate(all="ignore"):
        g = ((i + F32(0.5)) - F32(lo)) / (F32(hi) - F32(lo)) * F32(2) - F32(1)
        x = ((g + F32(1)) * F32(M) - F32(1)) * F32(0.5)
        fl = np.floor(x)
        return fl, ((fl + F32(1)) - x).astype(F32), (x - fl).astype(F32)


def paste_numpy(prob, box, H, W, threshold=0.5):
    """one mask: float32 probabilities [M, M], box (x0, y0, x1, y1) -> uint8 [H, W], in the kernel's operation order"""
    prob = np.asarray(prob, F32)
    M = prob.shape[0]
    x0, y0, x1, y1 = (F32(v) for v in box)
    out = np.zeros((H, W), np.uint8)
    if not np.isfinite([x0, y0, x1, y1]).all() or not (x1 > x0 and y1 > y0):
        return out
    cl = clip_boxes([x0, y0, x1, y1], H, W)[0]
    xs, xe, ys, ye = int(np.floor(cl[0])), int(np.ceil(cl[2])), int(np.floor(cl[1])), int(np.ceil(cl[3]))
    if xe <= xs or ye <= ys:
        return out
    xl, wx0, wx1 = _axis(W, x0, x1, M)
    yl, wy0, wy1 = _axis(H, y0, y1, M)
    pad = np.zeros((M + 2, M + 2), F32)                     # taps outside [0, M) read 0
    pad[1:-1, 1:-1] = prob
    okx, oky = (xl >= -1) & (xl <= M - 1), (yl >= -1) & (yl <= M - 1)
    xi, yi = np.where(okx, xl, 0).astype(np.int64) + 1, np.where(oky, yl, 0).astype(np.int64) + 1
    Y, X = yi[:, None], xi[None, :]
    with np.errstate(all="ignore"):
        nw, ne = (wx0[None, :] * wy0[:, None]).astype(F32), (wx1[None, :] * wy0[:, None]).astype(F32)
        sw, se = (wx0[None, :] * wy1[:, None]).astype(F32), (wx1[None, :] * wy1[:, None]).astype(F32)
        v = (((nw * pad[Y, X]).astype(F32) + (ne * pad[Y, X + 1]).astype(F32)).astype(F32) + (sw * pad[Y + 1, X]).astype(F32)).astype(F32)
        v = (v + (se * pad[Y + 1, X + 1]).astype(F32)).astype(F32)
        bit = (v >= F32(threshold)) & okx[None, :] & oky[:, None]
    out[ys:ye, xs:xe] = bit[ys:ye, xs:xe]
    return out


def probs_numpy(logits, classes):
    """mask_rcnn_inference: [N, C, M, M] logits (any float array) -> float32 probabilities [N, M, M] of the predicted class's channel"""
    logits = np.asarray(logits, F32)
    if logits.shape[1] == 1:
        return sigmoid_f32(logits[:, 0])
    return sigmoid_f32(logits[np.arange(len(logits)), np.asarray(classes, np.int64)])


def paste_masks_numpy(logits, boxes, classes, H, W, threshold=0.5):
    p = probs_numpy(logits, classes)
    return np.stack([paste_numpy(p[k], boxes[k], H, W, threshold) for k in range(len(p))]) if len(p) else np.zeros((0, H, W), np.uint8)


def paste_torch(prob, boxes, H, W, dtype=None):
    """Detectron2's _do_paste_mask (skip_empty=False) on the CPU: [N, M, M] probabilities, [N, 4] boxes -> the sampled values [N, H, W]
    (the caller thresholds).  dtype: torch.float32 (what the reference runs) or torch.float64 (what the band rule measures against)"""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float32
    masks = torch.as_tensor(np.asarray(prob)).to(dtype)[:, None]
    boxes = torch.as_tensor(np.asarray(boxes)).to(dtype)
    x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
    N = masks.shape[0]
    img_y = torch.arange(0, H, dtype=dtype) + 0.5
    img_x = torch.arange(0, W, dtype=dtype) + 0.5
    img_y = (img_y - y0) / (y1 - y0) * 2 - 1
    img_x = (img_x - x0) / (x1 - x0) * 2 - 1
    gx = img_x[:, None, :].expand(N, img_y.size(1), img_x.size(1))
    gy = img_y[:, :, None].expand(N, img_y.size(1), img_x.size(1))
    grid = torch.stack([gx, gy], dim=3)
    return F.grid_sample(masks, grid.to(masks.dtype), align_corners=False)[:, 0].numpy()


def band_check(got, prob, boxes, H, W, threshold=0.5, what=""):
    """The band rule: `got` [N, H, W] may differ from the float64 grid_sample of the float32 probabilities only where the float64
    value lies within BAND of the threshold, and such pixels are at most BAND_CAP of the pixels with a non-zero float64 value.
    The bound is derived: for boxes >= 4 px in frames <= 130 px float32 moves the sample coordinate by at most 2^-24 * 130 / 4 * 28
    ~ 5e-5 mask pixels, probabilities have slope <= 1 per mask pixel, and the four-tap sum adds a few 1e-7.  Prints and returns the count."""
    v = paste_torch(np.asarray(prob, np.float64), np.asarray(boxes, np.float64), H, W, dtype=__import__("torch").float64)
    want = v >= threshold
    band = np.abs(v - threshold) <= BAND
    bad = (np.asarray(got) != 0) != want
    n_band, n_pos = int(band.sum()), int((v != 0).sum())
    print(f"band rule {what}: {n_band} of {n_pos} non-zero pixels in the band, {int(bad.sum())} differ")
    assert not (bad & ~band).any(), f"{what}: {int((bad & ~band).sum())} pixels differ outside the band"
    assert n_band <= BAND_CAP * max(n_pos, 1), f"{what}: {n_band} of {n_pos} pixels in the band"
    return n_band


# ---------------------------------------------------------------------------------------------------------------- records
def scale_ratio(o, i):
    return F32(float(o) / float(i))


def postprocess_numpy(boxes, in_size, out_size):
    """detector_postprocess on the boxes: (scaled and clipped float32 [n, 4], keep bool [n])"""
    b = np.array(boxes, dtype=F32).reshape(-1, 4)
    sx, sy = scale_ratio(out_size[1], in_size[1]), scale_ratio(out_size[0], in_size[0])
    b = (b * np.array([sx, sy, sx, sy], dtype=F32)).astype(F32)
    b = clip_boxes(b, out_size[0], out_size[1])
    return b, ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)


def records_numpy(items, logits, in_sizes, out_sizes, image_ids, category_ids=None, threshold=0.5):
    """coco_records on the host; items: per image (boxes, scores, classes) arrays; logits [sum n, C, M, M] or None"""
    out, at = [], 0
    for (boxes, scores, classes), ins, outs, iid in zip(items, in_sizes, out_sizes, image_ids):
        b, keep = postprocess_numpy(boxes, ins, outs)
        mine = []
        for i in range(len(b)):
            if keep[i]:
                c = int(classes[i])
                r = {"image_id": iid, "category_id": c if category_ids is None else category_ids[c],
                     "bbox": [float(b[i, 0]), float(b[i, 1]), float(F32(b[i, 2] - b[i, 0])), float(F32(b[i, 3] - b[i, 1]))],
                     "score": float(F32(scores[i]))}
                if logits is not None:
                    p = probs_numpy(logits[at + i:at + i + 1], [c])[0]
                    r["segmentation"] = rle.encode_numpy(paste_numpy(p, b[i], outs[0], outs[1], threshold))
                mine.append(r)
        out.append(mine)
        at += len(b)
    return out


# ---------------------------------------------------------------------------------------------------------------- builders
def smooth_logits(rng, n, C, M):
    """5 x 5 normal noise x 6, upsampled bilinearly to M x M: float32 [n, C, M, M]"""
    import torch
    import torch.nn.functional as F
    z = torch.from_numpy((rng.standard_normal((n, C, 5, 5)) * 6).astype(np.float32))
    return F.interpolate(z, size=(M, M), mode="bilinear", align_corners=False).numpy().astype(F32)


def blob_logits(rng, n, C, M):
    """a soft disc per mask: +6 inside, -6 outside, a ramp of about two mask pixels between"""
    yy, xx = np.mgrid[0:M, 0:M].astype(np.float64) + 0.5
    out = np.empty((n, C, M, M), F32)
    for i in range(n):
        for c in range(C):
            cx, cy = rng.uniform(0.35, 0.65, 2) * M
            rad = rng.uniform(0.25, 0.4) * M
            d = np.hypot(xx - cx, yy - cy)
            out[i, c] = np.clip((rad - d) * 3.0, -6, 6)
    return out


def random_boxes(rng, n, H, W, min_side=4.0):
    x0, y0 = rng.uniform(-0.1 * W, 0.8 * W, n), rng.uniform(-0.1 * H, 0.8 * H, n)
    w, h = rng.uniform(min_side, 0.6 * W, n), rng.uniform(min_side, 0.6 * H, n)
    return np.stack([x0, y0, x0 + w, y0 + h], axis=1).astype(F32)


def selection_batch(seed, K, class_specific, rows=(0, 1, 63, 65, 300, 1100)):
    """the ragged batch of the GPU test: per image (boxes [R, 4 or 4K], scores [R, K + 1], (h, w)); image 2 passes nothing at
    score_thresh 0.05; the others carry the planted cases"""
    rng = np.random.RandomState(seed)
    shapes = [(40, 60), (37, 53), (64, 48), (96, 130), (80, 100), (120, 90)]
    out = []
    for k, R in enumerate(rows):
        h, w = shapes[k % len(shapes)]
        BC = K if class_specific else 1
        cx, cy = rng.uniform(0, w, (R, BC)), rng.uniform(0, h, (R, BC))
        bw, bh = rng.uniform(4, 0.35 * w, (R, BC)), rng.uniform(4, 0.35 * h, (R, BC))
        boxes = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=2).astype(F32)      # [R, BC, 4]
        raw = rng.uniform(0, 1, (R, K + 1))
        scores = (raw / raw.sum(axis=1, keepdims=True)).astype(F32)
        if k == 2:
            scores[:, :K] = F32(0.01) * scores[:, :K]                          # nothing passes 0.05
        if R >= 63 and k != 2:
            boxes[0, :], boxes[1, :] = [0, 0, 3, 1], [1, 0, 4, 1]              # IoU exactly 0.5
            scores[0, 0], scores[1, 0] = 0.97, 0.96
            boxes[3] = boxes[2]                                                # a duplicated box
            scores[2, 0], scores[3, 0] = 0.9995, 0.999
            scores[10:20, 0] = 0.5                                             # runs of equal scores
            scores[30:34, K - 1] = 0.25
            boxes[40, 0, 1] = np.nan
            boxes[41, BC - 1, 2] = np.inf
            scores[42, K] = np.nan                                             # the background column counts too
            scores[43, 0] = -np.inf
            boxes[44, :] = [w + 5, 2, w + 20, 12]                              # wholly outside: clips to zero area
            boxes[45, :] = [w + 8, 3, w + 25, 14]
            boxes[46, :] = [-30, -30, -5, -2]
            scores[44:47, 0] = [0.93, 0.92, 0.91]
            scores[50, 0] = 0.05                                               # equal to the threshold: dropped
        out.append((boxes.reshape(R, BC * 4), scores, (h, w)))
    return out


def load_fixture():
    return np.load(os.path.join(HERE, "golden", "det_post.npz"), allow_pickle=False)


def ranked_image(boxes):
    """one image of one class whose candidates are `boxes` in this order: score 1 - r / 1024 for row r (exact, above 0.05 for r < 972)"""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    n = len(boxes)
    assert n < 972
    scores = np.zeros((n, 2), F32)
    scores[:, 0] = F32(1) - np.arange(n, dtype=F32) / F32(1024)
    return boxes, scores, (64, 65536)


# the class predicate: (rows, classes) kept of class_pairs' two images, in output order
CLASS_PAIRS_KEPT = ([(0, 0), (0, 1)], [(0, 0)])


def class_pairs(class_specific):
    """two images of K = 2 classes.  The first: one row that passes under both classes with the same box -- two candidates that overlap
    fully and differ in class, both kept.  The second: two rows with that box under class 0 alone -- one kept."""
    box = np.array([10, 10, 50, 40], F32)
    reps = 2 if class_specific else 1
    one = (np.tile(box, (1, reps)), np.array([[0.9, 0.8, 0.0]], F32), (64, 64))
    two = (np.tile(box, (2, reps)), np.array([[0.9, 0.01, 0.0], [0.8, 0.02, 0.0]], F32), (64, 64))
    return [one, two]


def many_candidates(R, K, seed=7):
    """one image whose R x K (row, class) pairs all pass 0.05: boxes 20 to 60 px per side around centres in a 200 x 200 frame, so that a greedy NMS at
    0.5 keeps several hundred per class; class-agnostic boxes [R, 4], scores [R, K + 1]"""
    rng = np.random.RandomState(seed + R + K)
    c, wh = rng.uniform(0, 200, (R, 2)), rng.uniform(20, 60, (R, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], axis=1).astype(F32)
    scores = np.concatenate([rng.uniform(0.06, 1, (R, K)), np.zeros((R, 1))], axis=1).astype(F32)
    return boxes, scores, (240, 240)
