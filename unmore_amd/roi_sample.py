"""The first step of the stage-3 detector's cascade ROI heads in training on the device: Detectron2's ROIHeads.label_and_sample_proposals
(cad/modeling/roi_heads/roi_heads.py:207-328, called by CustomCascadeROIHeads.forward) with add_ground_truth_to_proposals, the matcher,
subsample_labels and the gathers of every gt_* field, and select_foreground_proposals (roi_heads.py:66-95) as a prefix view.

  label_and_sample_proposals    append, match, sample, order and gather for the whole batch: the upload of one table and two launches
  add_ground_truth_to_proposals the append alone (torch.cat per image)
  foreground                    the foreground rows of every image: views, no nonzero

The semantics (tests/roi_sample_common.py restates them in NumPy; csrc/roi_sample.hip writes the arithmetic out):
  1. Append.  With proposal_append_gt image i's candidates are its R_i proposals followed by its G_i ground-truth boxes; a ground truth's
     objectness logit is float32(log((1 - 1e-10) / (1 - (1 - 1e-10)))) evaluated in Python floats (Detectron2's value).  The kernels read
     the two sources in place; candidate index r runs over [0, R_i + G_i).
  2. Match.  IoU = box_loss's pairwise_iou (float32, every operation rounded on its own, 0 unless inter > 0: the float32 NumPy value
     bit for bit).  Per candidate the maximum over the image's ground truths at the LOWEST index that attains it; foreground iff the
     maximum >= float32(iou_threshold): Matcher([t], [0, 1], allow_low_quality_matches=False).  Class: gt_classes[matched] for
     foreground, num_classes for background.  An image without ground truths: everything background, matched index 0.
  3. Pools.  subsample_labels: positive iff class != -1 and != num_classes (P of them), negative iff class == num_classes (Q);
     num_pos = min(P, int(B * positive_fraction)), num_neg = min(Q, B - num_pos), B = batch_size_per_image.
  4. Draw.  The num_pos positives with the LARGEST key are taken, equal keys to the lower r; likewise the negatives.  Keys are 31-bit
     non-negative integers: `keys`, a list of int32 [R_i + G_i] device tensors or one flat tensor of all images' (only the low 31 bits
     count), with which a caller imposes any order; or, by default, rpn_loss's stateless hash of (seed', image, r) with
     seed' = seed ^ 0x726f695f68656164, so that the same per-step seed given to both samplers yields unrelated keys.  This is a uniform
     sample without replacement like subsample_labels' randperm(P)[:k]; it is NOT torch's randperm draw, consumes no device RNG state and
     reads nothing back.
  5. Order.  "key" (default): the foreground samples by descending key, ties to the lower r, then the background samples likewise -- a
     uniformly random order like the reference's positive[perm]; the reference goes by row position afterwards
     (custom_cascade_rcnn.py:205, 223: the first 100 rows, the single-object flag).  "index": ascending r inside each part.
  6. Outputs per image, views into one flat buffer per field: proposal_boxes [S_i,4], objectness_logits, gt_classes int64, gt_boxes
     (gathered by matched index on EVERY row, background included), gt_scores (when the targets have them), matched_idxs int64 with
     mask_index the same tensor, sampled_idxs int32 (the r of each row), gt_masks passed through (never gathered: mask_loss reads them
     through mask_index); S_i = num_pos + num_neg.

Departures from the reference, on purpose:
  * a candidate with a non-finite coordinate is never sampled and is counted `bad` (Detectron2's Matcher would label its NaN IoU 1);
  * a NaN IoU that comes from a ground truth never wins the maximum, as in box_loss.match_and_label;
  * an image without ground truths gets zero gt_boxes / gt_scores (and matched_idxs 0); the reference sets no gt_* fields there.

Limits (ValueError before any launch): R_i + G_i <= 16384 per image, batch_size_per_image <= 1024, 1 <= N <= 65535, float32 boxes, one
device, a threshold that is a number.  Out of scope: matchers with an ignore band, keypoints, rotated boxes.  No CPU fallback."""
import math

import numpy as np
import torch

from . import _lib as L
from . import _tables as T
from .ops import _p, _stream

CHUNK = 256                  # candidates per workgroup of the match launch (csrc/roi_sample.hip: RS_THREADS)
MAX_BATCH = 1024             # RS_MAX_BATCH
MAX_CANDIDATES = 16384       # RS_MAX_CANDIDATES: proposals and appended ground truths of one image
FIELDS = 11                  # RS_FIELDS: int64 per image of the table
SEED_SALT = 0x726f695f68656164
GT_LOGIT = math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10)))      # add_ground_truth_to_proposals' logit of a ground truth
COUNTERS = ("positives", "negatives", "sampled_fg", "sampled_bg", "bad")
ROW_FIELDS = ("proposal_boxes", "objectness_logits", "gt_classes", "gt_boxes", "gt_scores", "matched_idxs", "mask_index", "sampled_idxs")


class Samples(list):
    """label_and_sample_proposals' list form: one dict per image, and what `foreground` needs -- `counts`, the (num_pos, num_neg) pairs
    read from the device, `counts_device` int32 [N,2], and `padded`, the [N,B,...] buffers the dicts are views of"""
    counts = counts_device = padded = None


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _pair(item, k):
    """(proposal_boxes, objectness_logits) of proposals[k]: a dict, an object with those fields, or rpn_proposals' (boxes, logits)"""
    if isinstance(item, (tuple, list)) and len(item) == 2:
        boxes, logits = item
    else:
        get = T.getter(item)
        boxes, logits = get("proposal_boxes"), get("objectness_logits")
    boxes = T.unwrap(boxes)
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError(f"roi_sample: proposals[{k}]: proposal_boxes must be float32 [R, 4], got {getattr(boxes, 'dtype', type(boxes))} "
                         f"{list(getattr(boxes, 'shape', []))}")
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or tuple(logits.shape) != (boxes.shape[0],):
        raise ValueError(f"roi_sample: proposals[{k}]: objectness_logits must be float32 [{int(boxes.shape[0])}], got "
                         f"{getattr(logits, 'dtype', type(logits))} {list(getattr(logits, 'shape', []))}")
    return boxes, logits


def _target(item, k):
    """(gt_boxes, gt_classes, gt_scores or None, gt_masks or None) of targets[k]"""
    get = T.getter(item)
    gtb, gtc, gts = T.unwrap(get("gt_boxes")), get("gt_classes"), get("gt_scores")
    if not isinstance(gtb, torch.Tensor) or gtb.dtype != torch.float32 or gtb.dim() != 2 or gtb.shape[1] != 4:
        raise ValueError(f"roi_sample: targets[{k}]: gt_boxes must be float32 [G, 4], got {getattr(gtb, 'dtype', type(gtb))} "
                         f"{list(getattr(gtb, 'shape', []))}")
    n = int(gtb.shape[0])
    if not isinstance(gtc, torch.Tensor) or tuple(gtc.shape) != (n,) or gtc.dtype.is_floating_point or gtc.dtype.is_complex or \
            gtc.dtype == torch.bool:
        raise ValueError(f"roi_sample: targets[{k}]: gt_classes must be integer [{n}], got {getattr(gtc, 'dtype', type(gtc))} "
                         f"{list(getattr(gtc, 'shape', []))}")
    if gts is not None and (not isinstance(gts, torch.Tensor) or gts.dtype != torch.float32 or tuple(gts.shape) != (n,)):
        raise ValueError(f"roi_sample: targets[{k}]: gt_scores must be float32 [{n}], got {getattr(gts, 'dtype', type(gts))} "
                         f"{list(getattr(gts, 'shape', []))}")
    return gtb, gtc, gts, get("gt_masks")


def _lists(proposals, targets):
    proposals, targets = list(proposals), list(targets)
    N = len(proposals)
    if not 1 <= N <= 65535:
        raise ValueError(f"roi_sample: proposals: between 1 and 65535 images, got {N}")
    if len(targets) != N:
        raise ValueError(f"roi_sample: targets: one per image, got {len(targets)} for {N} images")
    return [_pair(p, k) for k, p in enumerate(proposals)], [_target(t, k) for k, t in enumerate(targets)]


def add_ground_truth_to_proposals(targets, proposals):
    """Detectron2's add_ground_truth_to_proposals: per image (boxes float32 [R_i + G_i, 4], logits float32 [R_i + G_i]), the proposals
    followed by the ground-truth boxes with the logit GT_LOGIT: one torch.cat per field and image, on whichever device the tensors are.
    label_and_sample_proposals does NOT call it: its kernels read the two sources in place."""
    props, tgts = _lists(proposals, targets)
    out = []
    for (boxes, logits), (gtb, _, _, _) in zip(props, tgts):
        if boxes.device != gtb.device:
            raise ValueError(f"roi_sample: every tensor must be on the same device, got {sorted({str(boxes.device), str(gtb.device)})}")
        out.append((torch.cat([boxes, gtb]), torch.cat([logits, logits.new_full((int(gtb.shape[0]),), GT_LOGIT)])))
    return out


def label_and_sample_proposals(proposals, targets, *, iou_threshold=0.5, num_classes=1, batch_size_per_image=512, positive_fraction=0.25,
                               proposal_append_gt=True, seed=0, keys=None, order="key", padded=False, stats=None, _phase_ms=None,
                               _alloc=None):
    """Detectron2's ROIHeads.label_and_sample_proposals for the whole batch; the module docstring lists the steps and the departures.

    proposals: one item per image, a dict or an object with `proposal_boxes` float32 [R_i,4] (`.tensor` unwrapped) and
    `objectness_logits` float32 [R_i], or rpn.rpn_proposals' (boxes, logits) pair.  targets: one item per image with `gt_boxes` float32
    [G_i,4], `gt_classes` integer [G_i], optionally `gt_scores` float32 [G_i] (all targets or none: without it no `gt_scores` comes
    back) and `gt_masks` (passed through).  seed: a Python int per step; keys: see the module docstring; order: "key" or "index".

    Returns a Samples list with one dict per image (ROW_FIELDS, every tensor a view into one [N,B,...] buffer per field, and `gt_masks`
    when given), which goes unchanged into box_loss.fast_rcnn_losses, roi_pool.ROIPooler (its proposal_boxes), box_loss.match_and_label
    and mask_loss.mask_rcnn_loss_weighted.  The list form reads the int32 [N,2] counts once: the call's only host read.  padded=True
    returns instead a dict of the [N,B,...] buffers with `counts` int32 [N,2] = (num_pos, num_neg) on the device and reads nothing:
    rows past num_pos + num_neg are zero with gt_classes -1.

    stats: a dict that receives `counters`, int32 [N,5] ON THE DEVICE in the order of COUNTERS (P, Q, sampled foreground, sampled
    background, bad candidates), `scalars`, a function that reads them when called and gives Detectron2's logged
    roi_head/num_fg_samples and roi_head/num_bg_samples (means over the images) and `bad`, and `matched_idxs` int32 / `matched_vals`
    float32, per image the [R_i + G_i] results of the match launch for EVERY candidate (views into the call's workspace).  ValueError for argument errors before any
    launch, RuntimeError off the GPU.  The same input gives the same bytes.  _alloc: the tests' allocator (shape, dtype) -> tensor for
    every buffer the launches write, instead of torch.empty."""
    props, tgts = _lists(proposals, targets)
    N = len(props)
    try:
        t = float(iou_threshold)
    except (TypeError, ValueError):
        raise ValueError(f"roi_sample: iou_threshold must be a number, got {iou_threshold!r}") from None
    if math.isnan(t):
        raise ValueError("roi_sample: iou_threshold is NaN")
    if not _is_int(num_classes) or num_classes < 0:
        raise ValueError(f"roi_sample: num_classes must be a non-negative integer, got {num_classes!r}")
    if not _is_int(batch_size_per_image) or not 1 <= batch_size_per_image <= MAX_BATCH:
        raise ValueError(f"roi_sample: batch_size_per_image must be an integer in [1, {MAX_BATCH}], got {batch_size_per_image!r}")
    B = int(batch_size_per_image)
    try:
        frac = float(positive_fraction)
    except (TypeError, ValueError):
        raise ValueError(f"roi_sample: positive_fraction must be a number, got {positive_fraction!r}") from None
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"roi_sample: positive_fraction must lie in [0, 1], got {positive_fraction!r}")
    if not _is_int(seed):
        raise ValueError(f"roi_sample: seed must be an integer, got {seed!r}")
    if order not in ("key", "index"):
        raise ValueError(f"roi_sample: order must be 'key' or 'index', got {order!r}")
    append = bool(proposal_append_gt)
    sizes = []
    for k, ((boxes, _), (gtb, _, _, _)) in enumerate(zip(props, tgts)):
        R, G = int(boxes.shape[0]), int(gtb.shape[0])
        if R + G > MAX_CANDIDATES:
            raise ValueError(f"roi_sample: proposals[{k}]: {R} proposals and {G} ground truths, more than {MAX_CANDIDATES} per image")
        sizes.append((R, G, G if append else 0))
    with_scores = [g[2] is not None for g in tgts]
    if any(with_scores) and not all(with_scores):
        raise ValueError("roi_sample: targets: gt_scores in every target or in none")
    cand = [r + a for r, _, a in sizes]
    if keys is not None:
        if isinstance(keys, torch.Tensor):
            if keys.dtype != torch.int32 or keys.dim() != 1 or int(keys.shape[0]) != sum(cand):
                raise ValueError(f"roi_sample: keys as one tensor must be int32 [{sum(cand)}], got {keys.dtype} {list(keys.shape)}")
            keys = list(keys.split(cand))
        keys = list(keys)
        if len(keys) != N:
            raise ValueError(f"roi_sample: keys: one tensor per image, got {len(keys)} for {N} images")
        for k, (kt, c) in enumerate(zip(keys, cand)):
            if not isinstance(kt, torch.Tensor) or kt.dtype != torch.int32 or tuple(kt.shape) != (c,):
                raise ValueError(f"roi_sample: keys[{k}] must be int32 [{c}], got {getattr(kt, 'dtype', type(kt))} "
                                 f"{list(getattr(kt, 'shape', []))}")
    tensors = [x for p in props for x in p] + [x for g in tgts for x in g[:3] if x is not None] + (keys or [])
    dev = T.one_device(tensors, "roi_sample", "label_and_sample_proposals")
    seed = ((int(seed) & ((1 << 64) - 1)) ^ SEED_SALT)
    seed = seed - (1 << 64) if seed >= 1 << 63 else seed
    pos_cap = int(B * frac)
    with torch.cuda.device(dev):
        table = np.zeros((N, FIELDS), dtype=np.int64)
        hold, chunk, first = [], 0, 0
        for k, ((boxes, logits), (gtb, gtc, gts, _), (R, G, A)) in enumerate(zip(props, tgts, sizes)):
            ts = [boxes.contiguous(), logits.contiguous(), gtb.contiguous(), gtc.to(torch.int64).contiguous(),
                  None if gts is None else gts.contiguous(), None if keys is None else keys[k].contiguous()]
            hold += ts
            table[k, :6] = [0 if x is None or x.numel() == 0 else x.data_ptr() for x in ts]
            table[k, 6:] = [R, G, A, chunk, first]
            chunk += (R + A + CHUNK - 1) // CHUNK
            first += R + A
        table_d = torch.from_numpy(table).to(dev)
        empty = _alloc if _alloc is not None else (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev))
        out = {"proposal_boxes": empty((N, B, 4), torch.float32), "objectness_logits": empty((N, B), torch.float32),
               "gt_classes": empty((N, B), torch.int64), "gt_boxes": empty((N, B, 4), torch.float32),
               "matched_idxs": empty((N, B), torch.int64), "sampled_idxs": empty((N, B), torch.int32)}
        if all(with_scores):
            out["gt_scores"] = empty((N, B), torch.float32)
        counts, counters = empty((N, 2), torch.int32), empty((N, 5), torch.int32)
        nbytes = L.lib().umr_roi_sample_workspace(first)
        ws = T.workspace(nbytes, dev) if _alloc is None else _alloc((max(16, (int(nbytes) + 15) // 16 * 16),), torch.uint8)

        def launch(phases):
            L.check(L.lib().umr_roi_sample(_p(table_d), N, first, chunk, t, int(num_classes), B, pos_cap, 1 if order == "key" else 0,
                                           GT_LOGIT, seed, phases, _p(out["proposal_boxes"]), _p(out["objectness_logits"]),
                                           _p(out["gt_classes"]), _p(out["gt_boxes"]), _p(out["gt_scores"]) if "gt_scores" in out else None,
                                           _p(out["matched_idxs"]), _p(out["sampled_idxs"]), _p(counts), _p(counters), _p(ws), nbytes,
                                           _stream()), "umr_roi_sample")
        T.timed(launch, (("match", 1), ("select", 2)), _phase_ms)
        del hold
    out["mask_index"] = out["matched_idxs"]
    out["counts"] = counts
    if stats is not None:
        def scalars():
            """Detectron2's logged counts, read from the device when asked"""
            c = counters.sum(dim=0).tolist()
            return {"roi_head/num_fg_samples": c[2] / N, "roi_head/num_bg_samples": c[3] / N, "bad": int(c[4])}
        slots = max(first, 1)                                              # the match launch's per-candidate results, in the workspace
        stats["counters"], stats["scalars"] = counters, scalars
        stats["matched_idxs"] = list(ws[:4 * slots].view(torch.int32)[:first].split(cand))
        stats["matched_vals"] = list(ws[4 * slots:8 * slots].view(torch.float32)[:first].split(cand))
    masks = [g[3] for g in tgts]
    if padded:
        if any(m is not None for m in masks):
            out["gt_masks"] = masks
        return out
    host = counts.tolist()                                                 # the call's only host read
    res = Samples()
    for k, (p, q) in enumerate(host):
        item = {name: out[name][k, :p + q] for name in ROW_FIELDS if name in out and name != "mask_index"}
        item["mask_index"] = item["matched_idxs"]
        if masks[k] is not None:
            item["gt_masks"] = masks[k]
        res.append(item)
    res.counts, res.counts_device, res.padded = host, counts, out
    return res


def foreground(samples):
    """select_foreground_proposals on label_and_sample_proposals' result: the foreground samples are the first rows of every image, so
    this is a list of dicts of views (every row field cut to its first num_pos rows, `gt_masks` passed on), without nonzero or a read.
    For the padded form: the bool [N,B] mask of the foreground rows (arange(B) < num_pos), computed on the device."""
    if isinstance(samples, Samples):
        out = []
        for item, (p, _) in zip(samples, samples.counts):
            fg = {name: (v[:p] if name in ROW_FIELDS else v) for name, v in item.items()}
            fg["mask_index"] = fg["matched_idxs"]
            out.append(fg)
        return out
    if isinstance(samples, dict) and isinstance(samples.get("counts"), torch.Tensor) and "gt_classes" in samples:
        B = int(samples["gt_classes"].shape[1])
        return torch.arange(B, device=samples["counts"].device)[None, :] < samples["counts"][:, :1]
    raise ValueError("roi_sample: foreground takes label_and_sample_proposals' result")
