"""Comparators for unmore_amd.mask_loss (shared by the CPU and GPU tests, the fixture's generator and tools/mask_loss_bench.py).

roi_align_average / mask_targets_np: the target rule of csrc/mask_loss.hip in plain NumPy -- torchvision's roi_align(spatial_scale 1,
sampling_ratio 0, aligned) of a 0 / 1 mask, which is what Detectron2's BitMasks.crop_and_resize runs before its `>= 0.5` -- in float32
with every operation rounded on its own and in the kernel's order, or in float64.
loss_reference: loss, counters and gradient of cad/modeling/roi_heads/roi_heads.py:1009-1045 in float64 torch ops.
blob_masks / tight_boxes / jittered_proposals / load_fixture: seeded inputs and tests/golden/mask_loss.npz."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_loss.npz")
MAX_COORD = float(1 << 20)


def _axis(lo, hi, M, size, dt):
    """the samples of one axis of one box: (low, high, l, h) as [M, grid] arrays, l = h = 0 for a sample outside [-1, size]; None for
    an empty grid.  start = lo - .5; roi = (hi - .5) - start; bin = roi / M; grid = ceil(roi / M);
    coordinate(p, i) = (start + p * bin) + ((i + .5) * bin) / grid"""
    lo, hi, half = dt(lo), dt(hi), dt(0.5)
    start = dt(lo - half)
    roi = dt(dt(hi - half) - start)
    if not roi > 0:
        return None
    bin_ = dt(roi / dt(M))
    grid = int(np.ceil(bin_))
    if grid < 1:
        return None
    p = np.arange(M, dtype=dt)[:, None]
    i = np.arange(grid, dtype=dt)[None, :]
    c = (start + p * bin_) + ((i + half) * bin_) / dt(grid)
    assert c.dtype == dt
    valid = (c >= -1) & (c <= size)
    c = np.where(c <= 0, dt(0), c)
    low = c.astype(np.int64)
    top = low >= size - 1
    low = np.where(top, size - 1, low)
    high = np.where(top, size - 1, low + 1)
    c = np.where(top, low.astype(dt), c)
    l = (c - low.astype(dt)).astype(dt)
    h = (dt(1) - l).astype(dt)
    low, high = np.where(valid, low, 0), np.where(valid, high, 0)
    return low, high, np.where(valid, l, dt(0)), np.where(valid, h, dt(0))


def roi_align_average(mask, box, M, dtype=np.float32):
    """[M, M] averages of one box over one mask (bool / 0-1 array [H, W]); samples summed iy-outer, ix-inner, one rounding per add"""
    dt = np.float32 if dtype == np.float32 else np.float64
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    ay, ax = _axis(box[1], box[3], M, H, dt), _axis(box[0], box[2], M, W, dt)
    if ay is None or ax is None:
        return np.zeros((M, M), dtype=dt)
    yl, yh, ly, hy = (a[:, None, :, None] for a in ay)
    xl, xh, lx, hx = (a[None, :, None, :] for a in ax)
    m = mask.astype(dt)
    val = (hy * hx) * m[yl, xl] + (hy * lx) * m[yl, xh] + (ly * hx) * m[yh, xl] + (ly * lx) * m[yh, xh]
    assert val.dtype == dt
    gh, gw = ay[0].shape[1], ax[0].shape[1]
    acc = np.cumsum(val.reshape(M, M, gh * gw), axis=2, dtype=dt)[:, :, -1]      # cumsum adds in order, in dt
    return (acc / dt(max(gh * gw, 1))).astype(dt)


def bad_proposals(boxes, mask_index, G):
    """what the kernel refuses: a mask index outside [0, G), a box coordinate that is not finite or beyond +-2^20"""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    idx = np.arange(boxes.shape[0]) if mask_index is None else np.asarray(mask_index).astype(np.int64)
    with np.errstate(invalid="ignore"):
        return (idx < 0) | (idx >= G) | ~(np.abs(boxes) <= MAX_COORD).all(1)


def mask_averages_np(masks, boxes, mask_index=None, side=28, dtype=np.float32):
    """one image: ([R, side, side] averages, [R] bad flags); a bad proposal's averages are zero"""
    masks, boxes = np.asarray(masks), np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    bad = bad_proposals(boxes, mask_index, masks.shape[0])
    idx = np.arange(boxes.shape[0]) if mask_index is None else np.asarray(mask_index).astype(np.int64)
    dt = np.float32 if dtype == np.float32 else np.float64
    out = np.zeros((boxes.shape[0], side, side), dtype=dt)
    for r in range(boxes.shape[0]):
        if not bad[r]:
            out[r] = roi_align_average(masks[idx[r]], boxes[r], side, dt)
    return out, bad


def mask_targets_np(masks, boxes, mask_index=None, side=28, dtype=np.float32):
    """bool [R, side, side]: BitMasks.crop_and_resize(boxes, side) of masks[mask_index]"""
    return mask_averages_np(masks, boxes, mask_index, side, dtype)[0] >= 0.5


def loss_reference(logits, targets, gt_classes=None, weights=None):
    """float64: (loss, counters int64 [4] = incorrect, positive, false positive, false negative, gradient [R,C,M,M]) of
    mask_rcnn_loss_weighted for given targets (bool [R,M,M]); weights None = ones"""
    x = torch.as_tensor(logits).detach().double().cpu().clone().requires_grad_(True)
    t = torch.as_tensor(targets).cpu().bool()
    R, C = x.shape[0], x.shape[1]
    if R == 0:
        return 0.0, np.zeros(4, dtype=np.int64), np.zeros(tuple(x.shape))
    sel = x[:, 0] if C == 1 else x[torch.arange(R), torch.as_tensor(gt_classes).cpu().long()]
    w = torch.ones(R, dtype=torch.float64) if weights is None else torch.as_tensor(weights).detach().double().cpu()
    loss = F.binary_cross_entropy_with_logits(sel, t.double(), weight=w[:, None, None], reduction="mean")
    loss.backward()
    wrong = (sel.detach() > 0) != t
    counters = np.array([int(wrong.sum()), int(t.sum()), int((wrong & ~t).sum()), int((wrong & t).sum())], dtype=np.int64)
    return loss.item(), counters, x.grad.numpy()


def logged_scalars(counters, n):
    """the reference's three logged scalars (:1024-1030) from the counters and the element count n = R * M * M"""
    inc, pos, fp, fn = (float(v) for v in counters[:4])
    return {"accuracy": 1 - inc / max(n, 1.0), "false_positive": fp / max(n - pos, 1.0), "false_negative": fn / max(pos, 1.0)}


def blob_masks(rng, H, W, G, r_min=0.08, r_max=0.45):
    """G elliptic blobs in an H x W frame, bool [G,H,W]"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    masks = np.zeros((G, H, W), dtype=bool)
    for k in range(G):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = max(rng.uniform(r_min, r_max) * H, 0.6), max(rng.uniform(r_min, r_max) * W, 0.6)
        masks[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return masks


def tight_boxes(masks):
    """BitMasks.get_bounding_boxes: [x_min, y_min, x_max + 1, y_max + 1], zeros for an empty mask; float32 [G,4]"""
    boxes = np.zeros((masks.shape[0], 4), dtype=np.float32)
    for k in range(masks.shape[0]):
        ys, xs = np.nonzero(masks[k])
        if ys.size:
            boxes[k] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return boxes


def jittered_proposals(rng, masks, n, jitter=0.15):
    """n proposals as a detector's foreground sampler leaves them: ground-truth boxes moved by up to `jitter` of their size;
    (boxes float32 [n,4], mask_index int64 [n])"""
    G = masks.shape[0]
    gt = tight_boxes(masks)
    idx = rng.randint(0, G, size=n).astype(np.int64) if G else np.zeros(0, dtype=np.int64)
    b = gt[idx].astype(np.float64)
    w, h = np.maximum(b[:, 2] - b[:, 0], 1.0), np.maximum(b[:, 3] - b[:, 1], 1.0)
    b += rng.uniform(-jitter, jitter, size=b.shape) * np.stack([w, h, w, h], 1)
    return b.astype(np.float32), idx


WIDTHS, HEIGHTS = (1, 63, 64, 65, 130), (1, 7, 48)
COUNTS = (40, 3, 0, 40, 1, 3, 40, 40, 3, 0, 40, 3, 1, 40, 3)          # proposals per frame: 257 in all
N_BOX_KINDS = 7


def make_box(rng, kind, H, W):
    """one box of the kind the GPU tests cycle through"""
    if kind == 0:                                   # random float box reaching up to 3 px outside the frame
        xs, ys = np.sort(rng.uniform(-3, W + 3, 2)), np.sort(rng.uniform(-3, H + 3, 2))
        return xs[0], ys[0], xs[1], ys[1]
    if kind == 1:                                   # integer-aligned
        x1, y1 = rng.randint(0, W), rng.randint(0, H)
        return x1, y1, rng.randint(x1 + 1, W + 1), rng.randint(y1 + 1, H + 1)
    if kind == 2:                                   # sub-pixel: grid 1, bin < 1
        x1, y1 = rng.uniform(0, W), rng.uniform(0, H)
        return x1, y1, x1 + rng.uniform(0.05, 0.9), y1 + rng.uniform(0.05, 0.9)
    if kind == 3:                                   # the frame, within a fraction of a pixel
        j = rng.uniform(-0.4, 0.4, 4)
        return j[0], j[1], W + j[2], H + j[3]
    if kind == 4:                                   # zero width
        x1, y1 = rng.uniform(0, W), rng.uniform(0, H)
        return x1, y1, x1, y1 + 2.5
    if kind == 5:                                   # negative width
        x1, y1 = rng.uniform(0, W), rng.uniform(0, H)
        return x1 + 1.5, y1, x1, y1 + 2.5
    x1 = W + 1.5 + rng.uniform(0, 4)                # fully outside the frame
    return x1, rng.uniform(0, H), x1 + rng.uniform(1, 9), H + rng.uniform(0, 3)


def ragged_batch(side, C, seed=11):
    """The GPU tests' batch: every width x every height, 257 proposals, G in (1, 5), the box kinds cycling, and three planted bad
    proposals (a NaN coordinate, a 1e9 coordinate, a mask index out of range).  Returns (images -- dicts of arrays masks / boxes /
    mask_index / gt_classes --, logits float32 [257,C,side,side], weights float32 [257], number of planted bad proposals).  Some
    images carry uint8 masks with 255 for set, some an int32 index."""
    rng = np.random.RandomState(seed + side)
    images, k, n_img = [], 0, 0
    for H in HEIGHTS:
        for W in WIDTHS:
            n, G = COUNTS[n_img], (1, 5)[n_img % 2]
            masks = blob_masks(rng, H, W, G, 0.15, 0.6)
            boxes = np.zeros((n, 4), dtype=np.float32)
            for r in range(n):
                boxes[r] = make_box(rng, k % N_BOX_KINDS, H, W)
                k += 1
            idx = rng.randint(0, G, size=n).astype(np.int64)
            if n_img == 3:
                boxes[7, 1] = np.nan
            if n_img == 6:
                boxes[11, 2] = 1e9
            if n_img == 10:
                idx[5] = G
            if n_img % 3 == 1:
                idx = idx.astype(np.int32)
            if n_img % 4 == 2:
                masks = masks.astype(np.uint8) * 255
            images.append({"masks": masks, "boxes": boxes, "mask_index": idx, "gt_classes": rng.randint(0, C, size=n).astype(np.int64)})
            n_img += 1
    R = sum(COUNTS)
    logits = (rng.standard_normal((R, C, side, side)) * 3).astype(np.float32)
    weights = rng.uniform(0.1, 1.0, size=R).astype(np.float32)
    weights[::17], weights[5::29] = 0.0, 2.0
    return images, logits, weights, 3


def load_fixture():
    """tests/golden/mask_loss.npz -> dict: `images` (list of dicts masks / boxes / mask_index / gt_classes), `side`, `weights`,
    `targets`, and per case name ("c1", "c3", "c1_unweighted"): logits, loss, scalars (accuracy, false_positive, false_negative), grad"""
    z = np.load(GOLDEN)
    n = int(z["n_images"])
    images = [{"masks": z[f"im{k}_masks"], "boxes": z[f"im{k}_boxes"], "mask_index": z[f"im{k}_mask_index"],
               "gt_classes": z[f"im{k}_gt_classes"]} for k in range(n)]
    out = {"images": images, "side": int(z["side"]), "weights": z["weights"], "targets": z["targets"], "cases": {}}
    for name in ("c1", "c3", "c1_unweighted"):
        out["cases"][name] = {"logits": z[f"{name}_logits"], "loss": float(z[f"{name}_loss"]), "scalars": z[f"{name}_scalars"],
                              "grad": z[f"{name}_grad"], "weighted": name != "c1_unweighted"}
    return out
