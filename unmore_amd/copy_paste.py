"""Copy-paste augmentation of the stage-3 detector's training batches on the device (cad/engine/train_loop.py:90-248,
CustomSimpleTrainer.copy_and_paste, which the reference's recipe turns on for every batch: cad/model_zoo/configs/unMORE-IN+COCO/
cascade_mask_rcnn_R_50_FPN.yaml:3-8,58).  `draw_params` makes the reference's random draws on the host, from the reference's two random
streams and in its order; `copy_and_paste` runs a whole batch of pairs through one sequence of launches (csrc/copy_paste.hip).  No CPU
fallback: tests/copy_paste_common.py restates the method in torch CPU ops."""
import random

import numpy as np

MAX_PIXELS = 1 << 24     # the keep test 2 * inter < area equals the reference's float32 inter / area < 0.5 while both counts are exact in float32


def draw_params(n_labeled, unlabeled_sizes, rate, random_num, min_ratio, max_ratio, py_random=random, np_random=np.random):
    """The random draws of train_loop.py:132-163 for a batch of pairs.  n_labeled[p]: the number of instances of pair p's labeled item;
    unlabeled_sizes[p]: (H, W) of its unlabeled image.  Returns one entry per pair: None (no copy) or (choice, ratio, h_new, w_new,
    h_shift, w_shift).  Per pair, in this order: py_random.random() (copy iff rate >= draw and there are instances);
    num_copy = 1 for one instance, else np_random.randint(1, max(1, n)) with random_num, n without; np_random.choice(n, num_copy,
    replace=False); py_random.uniform(min_ratio, max_ratio); w_new = int(ratio * W), h_new = int(ratio * H); py_random.randint(0, W -
    w_new), then py_random.randint(0, H - h_new).  A pair that does not copy consumes only the first draw.  py_random / np_random: the
    `random` module or a random.Random, `numpy.random` or a RandomState; the defaults are the global streams, as in the reference."""
    if len(n_labeled) != len(unlabeled_sizes):
        raise ValueError(f"draw_params: {len(n_labeled)} instance counts for {len(unlabeled_sizes)} unlabeled sizes")
    out = []
    for n, (hu, wu) in zip(n_labeled, unlabeled_sizes):
        n, hu, wu = int(n), int(hu), int(wu)
        draw = py_random.random()
        if rate >= draw and n > 0:
            num_copy = (1 if n == 1 else int(np_random.randint(1, max(1, n)))) if random_num else n
        else:
            num_copy = 0
        if n == 0 or num_copy == 0:
            out.append(None)
            continue
        choice = np.asarray(np_random.choice(n, num_copy, replace=False)).astype(np.int64)
        ratio = py_random.uniform(min_ratio, max_ratio)
        w_new, h_new = int(ratio * wu), int(ratio * hu)
        w_shift = py_random.randint(0, wu - w_new)
        h_shift = py_random.randint(0, hu - h_new)
        out.append((choice, ratio, h_new, w_new, h_shift, w_shift))
    return out


def _check_item(item, what):
    """shape and dtype checks of one item, without touching its data: (H, W, N)"""
    import torch
    for key in ("image", "masks", "boxes"):
        if key not in item or not isinstance(item[key], torch.Tensor):
            raise ValueError(f"copy_and_paste: {what} needs a tensor '{key}'")
    img, masks, boxes = item["image"], item["masks"], item["boxes"]
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[0] != 3 or img.shape[1] < 1 or img.shape[2] < 1:
        raise ValueError(f"copy_and_paste: {what}: image must be uint8 [3, H, W], got {img.dtype} {list(img.shape)}")
    H, W = int(img.shape[1]), int(img.shape[2])
    if masks.dtype not in (torch.bool, torch.uint8) or masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W):
        raise ValueError(f"copy_and_paste: {what}: masks must be bool or uint8 [N, {H}, {W}], got {masks.dtype} {list(masks.shape)}")
    N = int(masks.shape[0])
    if boxes.dtype != torch.float32 or tuple(boxes.shape) != (N, 4):
        raise ValueError(f"copy_and_paste: {what}: boxes must be float32 [{N}, 4], got {boxes.dtype} {list(boxes.shape)}")
    return H, W, N


def _check_params(prm, p, Nl, Hu, Wu):
    try:
        choice, ratio, h_new, w_new, h_shift, w_shift = prm
        choice = np.asarray(choice).astype(np.int64).reshape(-1)
        ratio, h_new, w_new, h_shift, w_shift = float(ratio), int(h_new), int(w_new), int(h_shift), int(w_shift)
    except (TypeError, ValueError):
        raise ValueError(f"copy_and_paste: params[{p}] must be None or (choice, ratio, h_new, w_new, h_shift, w_shift)") from None
    if Nl == 0:
        raise ValueError(f"copy_and_paste: params[{p}] copies from a labeled item without instances")
    if choice.size < 1 or choice.size > Nl or choice.min() < 0 or choice.max() >= Nl or np.unique(choice).size != choice.size:
        raise ValueError(f"copy_and_paste: params[{p}]: choice must hold 1..{Nl} distinct indices below {Nl}")
    if h_new < 1 or w_new < 1:
        raise ValueError(f"copy_and_paste: params[{p}]: zero-sized resize ({h_new} x {w_new}); the reference's F.interpolate raises here")
    if h_shift < 0 or w_shift < 0 or h_shift + h_new > Hu or w_shift + w_new > Wu:
        raise ValueError(f"copy_and_paste: params[{p}]: the {h_new} x {w_new} frame at ({h_shift}, {w_shift}) leaves the {Hu} x {Wu} image")
    if not np.isfinite(ratio):
        raise ValueError(f"copy_and_paste: params[{p}]: ratio is not finite")
    return choice, ratio, h_new, w_new, h_shift, w_shift


def copy_and_paste(labeled, unlabeled, params=None, *, rate=1.0, random_num=True, min_ratio=0.3, max_ratio=1.0, _phase_ms=None):
    """CustomSimpleTrainer.copy_and_paste(labeled, unlabeled) for a whole batch in one sequence of launches.  The reference pairs a batch
    with its own reverse, `copy_and_paste(copy.deepcopy(data[::-1]), data)` (an odd batch pairs its middle image with itself); here
    the inputs are never modified, so `copy_and_paste(data[::-1], data)` does the same.

    labeled / unlabeled: lists of dicts with `image` (uint8 [3,H,W]), `masks` (bool or uint8 [N,H,W], N may be 0) and `boxes` (float32
    [N,4] XYXY), all on the GPU; every pair may have its own sizes and counts.  params: what `draw_params` returns (None = draw now, from
    the global streams, with rate / random_num / min_ratio / max_ratio).  Returns one dict per pair: `image`, `masks` (bool), `boxes`,
    `source` (int64 [M,2] on the device: (0 = unlabeled / 1 = labeled, index in that item) of every output instance, so a caller can carry
    gt_classes and any other field), `params`, and `areas` (int64 [M] on the host: the output masks' pixel counts, which the call reads
    back anyway).  A pair that copies nothing -- no draw, or every copy rejected -- returns the unlabeled item's own tensors (`areas`
    is None).

    The reference's semantics, quirks included: the chosen masks and the labeled image are resized with F.interpolate(bilinear,
    align_corners=False) (mask: any tap with a non-zero weight set; image: float32, truncated to a byte) and pasted at (h_shift,
    w_shift).  Unlabeled image without instances: every copy is kept, and the boxes are the chosen boxes scaled by (W_u / W_l * ratio,
    H_u / H_l * ratio) with h_shift added to x0, x1 and w_shift to y0, y1 -- the reference swaps the two shifts (:191-194) and this
    keeps the swap.  Otherwise a copy is kept iff its overlap with every existing mask is below half of that mask's area; an existing
    mask of area 0 makes the reference's ratio NaN and rejects every copy; existing masks lose the pasted pixels, those left with area
    0 are dropped, the output is the surviving existing instances followed by the kept copies, and every box is recomputed from its
    mask as Detectron2's BitMasks.get_bounding_boxes does ([x_min, y_min, x_max + 1, y_max + 1]).

    One host-to-device copy carries the tables, one small device-to-host read brings back keep flags, areas and boxes -- the call's
    only synchronisation.  Argument errors are ValueError before any launch (sizes, dtypes, a zero-sized resize, an unlabeled image of
    2^24 pixels or more); off the GPU the call raises RuntimeError."""
    import torch
    if len(labeled) != len(unlabeled):
        raise ValueError(f"copy_and_paste: {len(labeled)} labeled items for {len(unlabeled)} unlabeled ones")
    P = len(unlabeled)
    shapes_l = [_check_item(it, f"labeled[{p}]") for p, it in enumerate(labeled)]
    shapes_u = [_check_item(it, f"unlabeled[{p}]") for p, it in enumerate(unlabeled)]
    if params is None:
        params = draw_params([s[2] for s in shapes_l], [s[:2] for s in shapes_u], rate, random_num, min_ratio, max_ratio)
    if len(params) != P:
        raise ValueError(f"copy_and_paste: {len(params)} params entries for {P} pairs")
    checked = [None] * P
    for p in range(P):
        Hu, Wu, _ = shapes_u[p]
        if params[p] is None:
            continue
        if Hu * Wu >= MAX_PIXELS:
            raise ValueError(f"copy_and_paste: unlabeled[{p}] has {Hu} x {Wu} >= 2^24 pixels: the integer keep test would no longer be the "
                             "reference's float32 one")
        if shapes_l[p][0] * shapes_l[p][1] >= 1 << 31:
            raise ValueError(f"copy_and_paste: labeled[{p}] has 2^31 pixels or more")
        checked[p] = _check_params(params[p], p, shapes_l[p][2], Hu, Wu)
    tensors = [t for it in list(labeled) + list(unlabeled) for t in (it["image"], it["masks"], it["boxes"])]
    if P and any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError("unmore_amd.copy_paste.copy_and_paste runs on the MI355X only (no CPU fallback); "
                           "tests/copy_paste_common.py::copy_paste_reference restates it on the host")
    if P == 0:
        return []
    dev = unlabeled[0]["image"].device
    if any(t.device != dev for t in tensors):
        raise ValueError("copy_and_paste: every tensor must be on the same device")
    from . import _lib as L
    from . import _tables as T
    from .ops import _p, _stream

    active = [p for p in range(P) if checked[p] is not None]
    if len(active) > 65535:
        raise ValueError(f"copy_and_paste: {len(active)} copying pairs in one call; the launch grid holds 65535")
    # ---- tables: one umr_cp_pair per active pair, then the choices
    tab = (L.CpPair * max(len(active), 1))()
    hold = []                                                    # contiguous views the table points into
    word_off = inter_off = row_off = choice_off = out_off = 0
    out_offs, choices = [], []
    max_wpm = max_nc = max_nu = 0
    for k, p in enumerate(active):
        choice, ratio, h_new, w_new, h_shift, w_shift = checked[p]
        (Hl, Wl, Nl), (Hu, Wu, Nu) = shapes_l[p], shapes_u[p]
        nc = int(choice.size)
        li, lm, lb = T.as_u8(labeled[p]["image"]), T.as_u8(labeled[p]["masks"]), labeled[p]["boxes"].contiguous()
        ui, um = T.as_u8(unlabeled[p]["image"]), T.as_u8(unlabeled[p]["masks"])
        hold += [li, lm, lb, ui, um]
        e = tab[k]
        e.l_image, e.l_masks, e.l_boxes, e.u_image = li.data_ptr(), lm.data_ptr(), lb.data_ptr(), ui.data_ptr()
        e.u_masks = um.data_ptr() if Nu else None
        e.Hl, e.Wl, e.Nl, e.Hu, e.Wu, e.Nu, e.nc = Hl, Wl, Nl, Hu, Wu, Nu, nc
        e.h_new, e.w_new, e.h_shift, e.w_shift = h_new, w_new, h_shift, w_shift
        e.rh, e.rw = float(np.float32(Hl) / np.float32(h_new)), float(np.float32(Wl) / np.float32(w_new))
        e.sx, e.sy = float(np.float32(1. * Wu / Wl * ratio)), float(np.float32(1. * Hu / Hl * ratio))       # :173-174, as torch rounds a Python scalar
        wpm = Hu * ((Wu + 63) // 64)
        e.word_off, e.inter_off, e.row_off, e.choice_off = word_off, inter_off, row_off, choice_off
        word_off += (nc + Nu + 1) * wpm
        inter_off += (nc + 1) * Nu
        row_off += nc + Nu
        choice_off += nc
        o_img = out_off
        o_msk = o_img + ((3 * Hu * Wu + 15) & ~15)
        out_off = o_msk + (((nc + Nu) * Hu * Wu + 15) & ~15)
        out_offs.append((o_img, o_msk))
        choices.append(choice.astype(np.int32))
        max_wpm, max_nc, max_nu = max(max_wpm, wpm), max(max_nc, nc), max(max_nu, Nu)
    with torch.cuda.device(dev):
        stats_h = boxes_dev = out = None
        if active:
            out = torch.empty(out_off, dtype=torch.uint8, device=dev)
            for k in range(len(active)):
                tab[k].out_image, tab[k].out_masks = out.data_ptr() + out_offs[k][0], out.data_ptr() + out_offs[k][1]
            buf, (o_choice,) = T.upload(tab, len(active), dev, [np.concatenate(choices)])  # the one host-to-device copy of the tables
            choice_dev = buf[o_choice:]
            res = torch.zeros(row_off * 6, dtype=torch.int32, device=dev)      # stats int32 [rows][2] | boxes f32 [rows][4]
            boxes_dev = res[row_off * 2:].view(torch.float32).view(row_off, 4)
            nbytes = L.lib().umr_copy_paste_workspace(word_off, inter_off)
            ws = T.workspace(nbytes, dev)

            def launch(phases):
                L.check(L.lib().umr_copy_paste(_p(buf), len(active), _p(choice_dev), choice_off, word_off, inter_off, row_off, max_wpm, max_nc,
                                               max_nu, phases, _p(res), _p(boxes_dev), _p(ws), nbytes, _stream()), "umr_copy_paste")
            T.timed(launch, (("resize_paste", 1), ("overlap", 2), ("compose", 4)), _phase_ms)      # tools/copy_paste_bench.py times the three parts
            stats_h = res[:row_off * 2].cpu().numpy().reshape(row_off, 2)      # the call's only synchronisation
        # ---- what the flags say: per pair the rows to gather and the sources, uploaded as one index buffer
        plans, idx_parts, n_idx = [None] * P, [], 0
        for k, p in enumerate(active):
            nc, Nu = int(tab[k].nc), shapes_u[p][2]
            st = stats_h[tab[k].row_off:tab[k].row_off + Nu + nc]
            kept = np.flatnonzero(st[Nu:, 0])
            if kept.size == 0:
                continue
            survive = np.flatnonzero(st[:Nu, 1] > 0)
            rows = np.concatenate([survive, Nu + kept]).astype(np.int64)
            src = np.concatenate([np.stack([np.zeros_like(survive), survive], 1),
                                  np.stack([np.ones_like(kept), checked[p][0][kept]], 1)]).astype(np.int64)
            plans[p] = (k, n_idx, rows.size, rows.size == Nu + nc, torch.from_numpy(st[rows, 1].astype(np.int64)))
            idx_parts += [rows + int(tab[k].row_off), rows, src.reshape(-1)]
            n_idx += 4 * rows.size
        for p in range(P):
            if plans[p] is None:
                Nu = shapes_u[p][2]
                j = np.arange(Nu, dtype=np.int64)
                plans[p] = (None, n_idx, Nu, True, None)
                idx_parts.append(np.stack([np.zeros_like(j), j], 1).reshape(-1))
                n_idx += 2 * Nu
        idx = torch.from_numpy(np.concatenate(idx_parts)).to(dev) if n_idx else torch.zeros(0, dtype=torch.int64, device=dev)
        results = []
        for p in range(P):
            k, o, m, whole, areas = plans[p]
            if k is None:
                u = unlabeled[p]
                results.append({"image": u["image"], "masks": u["masks"], "boxes": u["boxes"], "source": idx[o:o + 2 * m].view(m, 2),
                                "params": params[p], "areas": None})
                continue
            (Hu, Wu, Nu), nc = shapes_u[p], int(tab[k].nc)
            o_img, o_msk = out_offs[k]
            image = out[o_img:o_img + 3 * Hu * Wu].view(3, Hu, Wu)
            masks = out[o_msk:o_msk + (Nu + nc) * Hu * Wu].view(Nu + nc, Hu, Wu).view(torch.bool)
            r0 = int(tab[k].row_off)
            if whole:
                boxes = boxes_dev[r0:r0 + Nu + nc]
            else:
                masks, boxes = masks[idx[o + m:o + 2 * m]], boxes_dev[idx[o:o + m]]
            results.append({"image": image, "masks": masks, "boxes": boxes, "source": idx[o + 2 * m:o + 4 * m].view(m, 2), "params": params[p],
                            "areas": areas})
    del hold
    return results
