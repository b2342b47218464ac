"""Ground-truth synthesis on the device: the label half of the reference's dataset item
(datasets.py:158-159,171-222, the branch without random crop) for a batch of masks, one call instead of a cv2 / PyTorch
pipeline per image on the host."""
import torch

from . import _lib as L
from ._tables import upload, workspace
from .ops import _p, _stream, _need_gpu


def synthesize_labels(masks, object_centers=None, use_bg_sdf=True):
    """masks: [B,H,W] bool / integer / float tensor on the GPU (non-zero = object), already at the training resolution.
    object_centers: optional [B,2] (x, y) float tensor in the same pixel coordinates (the reference scales the centre of
    the pre-resize mask, datasets.py:171-173); None = bounding-box centre of each mask (datasets.py:158-159).
    Returns the reference's label dict (datasets.py:210-216) batched: 'center_field' [B,2,H,W] f32, 'saliency_mask'
    [B,H,W] f32 (0/1; the collate casts everything to float, datasets.py:70-75), 'sdf' [B,H,W] f32."""
    _need_gpu(masks)
    assert masks.dim() == 3
    B, H, W = masks.shape
    m8 = (masks != 0).to(torch.uint8).contiguous()
    dev = masks.device
    cen = None
    if object_centers is not None:
        cen = object_centers.to(dev, torch.float32).contiguous()
        assert cen.shape == (B, 2)
    cf = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    sal = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    sdf = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    ws_bytes = L.lib().umr_label_synthesis_workspace(B, H, W)
    ws = workspace(ws_bytes, dev)
    L.check(L.lib().umr_label_synthesis(_p(m8), _p(cen), _p(cf), _p(sal), _p(sdf), _p(ws), ws_bytes, B, H, W, int(bool(use_bg_sdf)),
                                        _stream()), "umr_label_synthesis")
    return {"center_field": cf, "saliency_mask": sal, "sdf": sdf}


# ---------------------------------------------------------------------------------------------------------------------
# The random-crop branch of the training item (datasets.py:144-190; __getitem__ always takes it, :109)
# ---------------------------------------------------------------------------------------------------------------------
import math

PRE_CROP_SIZE = 400  # datasets.py:103-104


def random_resized_crop_params(height, width, scale=(0.08, 1.0), ratio=(0.75, 1.33), generator=None):
    """torchvision.transforms.RandomResizedCrop.get_params (torchvision 0.14.1, the version README.md:25 names; called at
    datasets.py:167-168) restated: ten tries of (area fraction ~ U(scale), log aspect ~ U(log ratio)), then a position
    uniform over the placements that fit; falls back to the central crop closest to the ratio range.  Returns
    (top, left, h, w).  The torchvision package is absent from this image: the algorithm follows its published source, the
    random stream is torch's CPU generator as there (parity at this boundary is unpinned)."""
    area = height * width
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect = math.exp(torch.empty(1).uniform_(log_lo, log_hi, generator=generator).item())
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            i = int(torch.randint(0, height - h + 1, size=(1,), generator=generator).item())
            j = int(torch.randint(0, width - w + 1, size=(1,), generator=generator).item())
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def _crop_resize_batch(src, boxes, Ho, Wo, nearest):
    B, C, H, W = src.shape
    dst = torch.empty((B, C, Ho, Wo), dtype=src.dtype, device=src.device)
    bx = torch.as_tensor(boxes, dtype=torch.int32).reshape(B, 4).to(src.device)
    L.check(L.lib().umr_crop_resize_batch(_p(src), _p(bx), _p(dst), B, C, H, W, Ho, Wo, int(nearest), _stream()), "umr_crop_resize_batch")
    return dst


def resize_bilinear(x, Ho, Wo):
    """transforms.Resize((Ho, Wo), BILINEAR) on a float tensor [B,C,H,W] (no antialias, datasets.py:99,103)."""
    _need_gpu(x)
    x = x.contiguous().float()
    B, _, H, W = x.shape
    return _crop_resize_batch(x, [[0, 0, W, H]] * B, Ho, Wo, False)


def resize_nearest_u8(m, Ho, Wo):
    """transforms.Resize((Ho, Wo), NEAREST) on a mask [B,H,W] (any dtype; returned as u8 0/1, datasets.py:100,104)."""
    _need_gpu(m)
    m8 = (m != 0).to(torch.uint8).contiguous()
    B, H, W = m8.shape
    return _crop_resize_batch(m8.view(B, 1, H, W), [[0, 0, W, H]] * B, Ho, Wo, True).view(B, Ho, Wo)


def distance_transform(masks, normalize=True):
    """cv2.distanceTransform(u8, DIST_L2, 3) per mask [B,H,W] (distance to the nearest zero pixel), optionally divided by its
    maximum (datasets.py:162-163)."""
    _need_gpu(masks)
    m8 = (masks != 0).to(torch.uint8).contiguous()
    B, H, W = m8.shape
    out = torch.empty((B, H, W), dtype=torch.float32, device=m8.device)
    nbytes = L.lib().umr_distance_transform_workspace(B, H, W)
    ws = workspace(nbytes, m8.device)
    L.check(L.lib().umr_distance_transform(_p(m8), _p(out), _p(ws), nbytes, B, H, W, int(bool(normalize)), _stream()), "umr_distance_transform")
    return out


def synthesize_training_items(images, masks, image_size, scale=(0.08, 1.0), use_bg_sdf=True, generator=None, params=None):
    """A batch of the reference's training items (datasets.py:111-216 after file decoding, random_crop=True as __getitem__
    uses it) on the device.
    images: list of [3,h,w] float tensors in [0,1] on the GPU (sizes may differ); masks: list of [h,w] tensors (non-zero =
    object).  scale = (args.random_crop_scale_min, args.random_crop_scale_max) (train_objectness_net.py:813-814).
    params: optional list of (top, left, h, w) crop boxes in the 400x400 frame (tests); None = draw them with
    `random_resized_crop_params` from `generator` (torch CPU generator; None = the global one), one item after the other as a
    single-worker DataLoader would.
    Returns (images [B,3,S,S] f32, labels dict: 'center_field' [B,2,S,S], 'saliency_mask' [B,S,S], 'instance_mask' [B,S,S],
    'object_center' [B,2] (x, y), 'sdf' [B,S,S], all f32 as after the reference's collate) and the crop boxes used.
    Items whose 400x400 mask is empty get the resized image and all-zero labels (datasets.py:146-157)."""
    B, S, P = len(images), int(image_size), PRE_CROP_SIZE
    assert B == len(masks) and B > 0
    dev = images[0].device
    img400 = torch.cat([resize_bilinear(im.unsqueeze(0), P, P) for im in images])                 # datasets.py:144
    m400 = torch.cat([resize_nearest_u8(mk.unsqueeze(0), P, P) for mk in masks])                    # :145
    # bounding-box centre of the 400x400 mask (:158-159) and emptiness (:146-147) -- small reductions, done with torch
    mb = m400.bool()
    rows, cols = mb.any(dim=2), mb.any(dim=1)
    empty = ~rows.any(dim=1)
    ar = torch.arange(P, device=dev)
    big = P + 1
    y0 = torch.where(rows, ar, big).amin(dim=1).float(); y1 = torch.where(rows, ar, -1).amax(dim=1).float()
    x0 = torch.where(cols, ar, big).amin(dim=1).float(); x1 = torch.where(cols, ar, -1).amax(dim=1).float()
    cx, cy = (x0 + x1) / 2, (y0 + y1) / 2
    fg400 = distance_transform(m400, normalize=True)                                                # :162-164
    if params is None:
        params = [random_resized_crop_params(P, P, scale=scale, generator=generator) for _ in range(B)]   # :167-168
    assert len(params) == B
    pt = torch.tensor(params, dtype=torch.float32, device=dev)                                      # top, left, h, w
    boxes = [[l, t, l + w, t + h] for (t, l, h, w) in params]
    alld = torch.cat([img400, fg400.unsqueeze(1)], dim=1)                                           # image + sdf share the bilinear resize (:174,176)
    out = _crop_resize_batch(alld, boxes, S, S, False)
    m_s = _crop_resize_batch(m400.view(B, 1, P, P), boxes, S, S, True).view(B, S, S)                # :175
    img_s, fg_s = out[:, :3].contiguous(), out[:, 3].contiguous()
    # :180-182 -- (centre - offset) * (image_size / extent): the factor is a Python float there, applied as a float32 scalar
    fx = torch.tensor([S / w for (_, _, _, w) in params], dtype=torch.float64).to(torch.float32).to(dev)
    fy = torch.tensor([S / h for (_, _, h, _) in params], dtype=torch.float64).to(torch.float32).to(dev)
    ocx = (cx - pt[:, 1]) * fx
    ocy = (cy - pt[:, 0]) * fy
    centers = torch.stack([ocx, ocy], dim=1).contiguous()
    cf = torch.empty((B, 2, S, S), dtype=torch.float32, device=dev)
    sal = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    sdf = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    nbytes = L.lib().umr_label_synthesis_workspace(B, S, S)
    ws = workspace(nbytes, dev)
    L.check(L.lib().umr_label_synthesis_cropped(_p(m_s), _p(centers), _p(fg_s), _p(cf), _p(sal), _p(sdf), _p(ws), nbytes, B, S, S,
                                                int(bool(use_bg_sdf)), _stream()), "umr_label_synthesis_cropped")
    inst = m_s.float()
    if bool(empty.any()):   # datasets.py:146-157: image resized directly, all-zero labels
        e = empty.nonzero().flatten()
        img_s[e] = resize_bilinear(img400[e], S, S)
        cf[e] = 0; sal[e] = 0; sdf[e] = 0; inst[e] = 0; centers[e] = 0
    labels = {"center_field": cf, "saliency_mask": sal, "instance_mask": inst, "object_center": centers, "sdf": sdf}
    return img_s, labels, params


# ---------------------------------------------------------------------------------------------------------------------
# The existence classifier's training item (datasets.py:285-349, ImageNet_votecut_labeled_classifier_Dataset.__getitem__)
# ---------------------------------------------------------------------------------------------------------------------
import random

import numpy as np


def _ragged_upload(f32s, u8s, shapes, extra, dev):
    """One host-to-device copy: the umr_ragged_src table of a ragged batch followed by `extra` (int32 arrays).  Returns the
    device buffer (int32) and the element offsets of the extras in it."""
    n = len(shapes)
    tab = (L.RaggedSrc * n)()
    for k, (h, w) in enumerate(shapes):
        tab[k].f32 = f32s[k].data_ptr() if f32s[k] is not None else None
        tab[k].u8 = u8s[k].data_ptr() if u8s[k] is not None else None
        tab[k].H, tab[k].W = h, w
    buf, offs = upload(tab, n, dev, [np.asarray(e, dtype=np.int32) for e in extra])
    return buf.view(torch.int32), [o // 4 for o in offs]


def background_squares(full_masks):
    """datasets.py:304-313 for a ragged batch: full_masks is a list of [h,w] u8 tensors on the GPU (non-zero = object).  Returns
    int32 [B,5] = (x1, y1, x2, y2, ok) on the device: the largest background square around the first float32 maximum of the
    zero-border 3x3 chamfer transform of `mask == 0`; ok = 0 for an empty box.  One launch, no synchronisation."""
    if not all(m.is_cuda for m in full_masks):
        raise RuntimeError("unmore_amd.background_squares runs on the MI355X only (no CPU fallback); move the masks to the GPU")
    if not full_masks or any(m.dim() != 2 or m.dtype != torch.uint8 for m in full_masks):
        raise ValueError("background_squares: a non-empty list of [h,w] uint8 masks expected")
    dev = full_masks[0].device
    ms = [m.contiguous() for m in full_masks]
    shapes = [(int(m.shape[0]), int(m.shape[1])) for m in ms]
    n = len(ms)
    tab, _ = _ragged_upload([None] * n, ms, shapes, [], dev)
    max_w, max_px = max(w for _, w in shapes), max(h * w for h, w in shapes)
    nbytes = L.lib().umr_bg_square_workspace(n, max_px)
    ws = workspace(nbytes, dev)
    out5 = torch.empty((n, 5), dtype=torch.int32, device=dev)
    L.check(L.lib().umr_bg_square(_p(tab), _p(out5), _p(ws), nbytes, n, max_w, max_px, _stream()), "umr_bg_square")
    return out5


def synthesize_classifier_items(images, top1_masks, full_masks, image_size, coins=None, params=None, generator=None):
    """A batch of the existence classifier's training items (datasets.py:285-349 after the cv2.imread calls) on the device.
    images: list of [3,h,w] f32 tensors in [0,1] on the GPU (sizes differ between items); top1_masks / full_masks: lists of
    [h,w] u8 tensors holding the raw PNG values of the top-1 single-component mask (`mask_folder`) and of the full VoteCut
    mask (`full_mask_folder`).  A mask stored transposed is rotated by the caller (torch.rot90(mask, -1), :300-302).
    coins: list of bools, True = try the background branch (tests); None = `random.random() < 0.5` per item in item order
    (Python's `random`, :286-289, as a single-worker loader draws them).
    params: list of (top, left, h, w) or None per item (tests); None = `random_resized_crop_params(h, w, ratio=(3/4, 4/3),
    generator=generator)` (RandomResizedCrop's defaults, :338) for exactly the items that take the foreground branch, in
    item order -- items that succeed on the background branch draw nothing.
    Background branch (:304-321): the largest background square of the full mask (zero-border 3x3 chamfer transform, first
    float32 maximum, box = int(centre -/+ radius)), cropped from the image and resized bilinearly; label 0.  An empty box
    (a mask without background, or a maximum in row / column 0) falls through to the foreground branch (:324-325): there
    torchvision's resize raises on the empty crop -- read from the code, not executed (neither cv2 nor torchvision was
    available where this was written).
    Foreground branch (:335-346): image and top-1 mask / 255 cropped by the RandomResizedCrop box and resized bilinearly;
    label 1 if the resized mask sums to more than 1.
    Returns images [B,3,S,S] f32, class_labels [B,1] f32 and info = {'branch': int32 [B] (0 background / 1 foreground),
    'boxes': int32 [B,4] (x1, y1, x2, y2) in source pixels, 'mask_sum': f32 [B] (0 for background items)}, all on the device.
    The call reads the background pass's [B,5] box table back once; that is its only synchronisation."""
    B, S = len(images), int(image_size)
    if not (B > 0 and len(top1_masks) == B and len(full_masks) == B):
        raise ValueError("synthesize_classifier_items: images, top1_masks and full_masks are lists of the same, non-zero length")
    if not all(t.is_cuda for t in list(images) + list(top1_masks) + list(full_masks)):
        raise RuntimeError("unmore_amd.synthesize_classifier_items runs on the MI355X only (no CPU fallback); move images and masks to the GPU")
    dev = images[0].device
    imgs = [im.float().contiguous() for im in images]
    shapes = [(int(im.shape[1]), int(im.shape[2])) for im in imgs]
    for im, m1, mf, hw in zip(imgs, top1_masks, full_masks, shapes):
        if im.dim() != 3 or im.shape[0] != 3 or tuple(m1.shape) != hw or tuple(mf.shape) != hw or m1.dtype != torch.uint8 or mf.dtype != torch.uint8:
            raise ValueError("synthesize_classifier_items: items are ([3,h,w] float image, [h,w] uint8 top-1 mask, [h,w] uint8 full mask)")
    if coins is None:
        coins = [random.random() < 0.5 for _ in range(B)]                                             # :286-289
    if len(coins) != B or (params is not None and len(params) != B):
        raise ValueError("synthesize_classifier_items: coins / params hold one entry per item")
    # ---- background pass over the items whose coin says so
    bg = [b for b in range(B) if coins[b]]
    bg_box = {}
    if bg:
        out5 = background_squares([full_masks[b] for b in bg])
        for b, row in zip(bg, out5.cpu().tolist()):                                                   # the call's one synchronisation
            if row[4]:
                bg_box[b] = row[:4]
    # ---- boxes: background squares where they exist, RandomResizedCrop boxes for everything else, drawn in item order
    branch, boxes = [], []
    for b, (h, w) in enumerate(shapes):
        if b in bg_box:
            branch.append(0)
            boxes.append(bg_box[b])
            continue
        p = params[b] if params is not None and params[b] is not None else \
            random_resized_crop_params(h, w, ratio=(3.0 / 4.0, 4.0 / 3.0), generator=generator)      # :338
        top, left, ph, pw = (int(v) for v in p)
        branch.append(1)
        boxes.append([left, top, left + pw, top + ph])
    # ---- one crop + resize launch for the whole batch; the top-1 mask rides along on foreground items only
    m1s = [top1_masks[b].contiguous() if branch[b] else None for b in range(B)]
    tab, (o_box, o_br) = _ragged_upload(imgs, m1s, shapes, [boxes, branch], dev)
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    m_out = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    m_sum = torch.empty(B, dtype=torch.float32, device=dev)
    L.check(L.lib().umr_crop_resize_ragged(_p(tab), _p(tab[o_box:]), _p(out), _p(m_out), _p(m_sum), B, 3, S, S, _stream()),
            "umr_crop_resize_ragged")
    class_labels = (m_sum > 1).to(torch.float32).view(B, 1)                                           # :343-346; background items sum to 0
    info = {"branch": tab[o_br:o_br + B], "boxes": tab[o_box:o_br].view(B, 4), "mask_sum": m_sum}
    return out, class_labels, info
