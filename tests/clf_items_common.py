"""CPU restatement of the existence classifier's training item -- TEST INFRASTRUCTURE ONLY.

Restates `ImageNet_votecut_labeled_classifier_Dataset.__getitem__` (the reference's datasets.py:285-349) after its two
cv2.imread calls, line by line, from what oracle/labels_oracle.py provides (`distance_transform_3x3`,
`distance_transform_3x3_literal`, `resize`) plus numpy / torch.

Parity status: UNPINNED.  The reference class needs cv2 and torchvision; neither can be imported where this was written, so
the class itself has never been executed here and no fixture could be made from it.  What stands in for
`cv2.distanceTransform(u8, DIST_L2, 3)` is the oracle's restatement of OpenCV's published 3x3 chamfer algorithm; what
stands in for torchvision 0.14.1's tensor `Resize` / `RandomResizedCrop` is F.interpolate(bilinear, align_corners=False,
no antialias) on the cropped tensor.  The fall-through of an empty background crop to the foreground branch (:324-325: the
resize raises on an empty tensor) is read from the code.
"""
import numpy as np
import torch

from oracle import labels_oracle as LO


def bg_square(full_mask, pad=10, dt=LO.distance_transform_3x3):
    """datasets.py:298,304-313 for one decoded full VoteCut mask [h,w] u8: the largest background square.
    Returns (x1, y1, x2, y2) exactly as the reference computes them (no clamping: the slice :316 does that)."""
    mask = np.array(np.asarray(full_mask) > 0).astype(np.uint8)                                  # :298
    bg_mask = 1 - mask                                                                           # :304
    paded_bg_mask = np.pad(bg_mask, pad, mode="constant", constant_values=0)                     # :305 copyMakeBorder(…, value=0)
    bg_sdf = dt(paded_bg_mask)                                                                   # :306
    bg_sdf = bg_sdf[pad:-pad, pad:-pad]                                                          # :307
    assert bg_sdf.dtype == np.float32
    y_center, x_center = np.unravel_index(bg_sdf.argmax(), bg_sdf.shape)                         # :308
    center_radius = bg_sdf[y_center, x_center]                                                   # :309 (a float32 scalar)
    x1 = int(x_center - center_radius)                                                           # :310-313
    y1 = int(y_center - center_radius)
    x2 = int(x_center + center_radius)
    y2 = int(y_center + center_radius)
    # int64 -/+ float32 promotes to float64 in numpy; pin that reading
    assert x1 == int(float(x_center) - float(center_radius)) and y2 == int(float(y_center) + float(center_radius))
    return x1, y1, x2, y2


def zero_border_fixed(src):
    """The formulation the kernel uses: OpenCV's two passes (oracle: distance_transform_3x3) with the one-pixel border
    initialised to 0 instead of INT_MAX >> 2, on the unpadded source.  Returns the 16.16 fixed-point field (int64)."""
    HV, DG, INIT0 = LO.HV, LO.DG, LO.INIT0
    src = np.asarray(src) != 0
    H, W = src.shape
    jj = np.arange(W, dtype=np.int64) * HV
    tmp = np.empty((H, W), np.int64)
    prev = np.zeros(W + 2, np.int64)
    for i in range(H):
        c = np.minimum(np.minimum(prev[:-2] + DG, prev[1:-1] + HV), prev[2:] + DG)
        c[0] = min(c[0], 0 + HV)
        c = np.where(src[i], c, 0)
        row = np.minimum.accumulate(c - jj) + jj
        tmp[i] = row
        prev[1:-1] = row
    prev[:] = 0
    out = np.empty((H, W), np.int64)
    for i in range(H - 1, -1, -1):
        c = np.minimum(tmp[i], np.minimum(np.minimum(prev[2:] + DG, prev[1:-1] + HV), prev[:-2] + DG))
        c[-1] = min(c[-1], 0 + HV)
        row = np.minimum.accumulate((c + jj)[::-1])[::-1] - jj
        prev[1:-1] = row
        out[i] = np.minimum(row, INIT0)
    return out


def zero_border_field(src):
    """zero_border_fixed as the float32 field cv2 returns: fixed * 2^-16 rounded to float32"""
    return zero_border_fixed(src).astype(np.float32) * np.float32(1.0 / 65536.0)


def bg_square_zero_border(full_mask):
    """(x1, y1, x2, y2, ok) as the kernel is specified: zero-border transform of `mask == 0`, first float32 maximum in raster
    order, float64 corner arithmetic truncated toward zero, clamped to the image as numpy slicing clamps"""
    bg = np.asarray(full_mask) == 0
    H, W = bg.shape
    f = zero_border_field(bg)
    y, x = np.unravel_index(f.argmax(), f.shape)
    r = float(f[y, x])
    x1, y1, x2, y2 = int(x - r), int(y - r), int(x + r), int(y + r)
    x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, W), min(y2, H)
    return x1, y1, x2, y2, int(x2 > x1 and y2 > y1)


def classifier_item(image, top1_mask, full_mask, coin, params, image_size, pad=10):
    """datasets.py:285-349 for one decoded item.  image [3,h,w] f32 in [0,1] (the reference's to_tensor output), top1_mask /
    full_mask [h,w] u8 (raw PNG values), coin = the outcome of `random.random() < 0.5` (:286-289), params = (top, left, h, w)
    of RandomResizedCrop.get_params for the foreground branch (the draw itself is outside this restatement).
    Returns (image [3,S,S] f32, class_label float, info) with info = {'branch', 'box' (x1, y1, x2, y2 as the slices see
    them), 'mask_sum' (float64 sum of the resized mask, 0.0 on the background branch), 'mask' ([S,S] or None)}."""
    S = image_size
    h, w = full_mask.shape
    if coin:                                                                                     # :293
        try:
            x1, y1, x2, y2 = bg_square(full_mask.numpy(), pad)                                   # :298-313
            crop = image[:, y1:y2, x1:x2]                                                        # :316 (HWC there, CHW here)
            out = LO.resize(crop, (S, S))                                                        # :318-319; raises on an empty crop
            box = (min(x1, w), min(y1, h), min(x2, w), min(y2, h))                               # what the slice kept
            return out, 0.0, {"branch": 0, "box": box, "mask_sum": 0.0, "mask": None}            # :321-323
        except Exception:                                                                        # :324-325
            pass
    mask = top1_mask.float().unsqueeze(0) / 255                                                  # :336 to_tensor(u8)
    top, left, ch, cw = params
    image_and_mask = torch.cat([image, mask], dim=0)                                             # :339
    image_and_mask = LO.resize(image_and_mask[:, top:top + ch, left:left + cw], (S, S))          # RandomResizedCrop: crop + bilinear
    out = image_and_mask[0:3]                                                                    # :341-342
    mask = image_and_mask[3:]
    class_label = 1.0 if mask.sum() > 1 else 0.0                                                 # :343-346
    return out, class_label, {"branch": 1, "box": (left, top, left + cw, top + ch), "mask_sum": float(mask.double().sum()),
                              "mask": mask[0]}
