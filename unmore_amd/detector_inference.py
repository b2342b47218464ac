"""The inference tail of the stage-3 detector on the device: from the heads' raw outputs to the per-image COCO result records that
coco_eval.COCOEvaluator.process and evaluate_ap consume, and that the self-training recipe writes back as the next round's pseudo-labels.
The reference does it in cad/modeling/roi_heads/fast_rcnn.py:52-179 (fast_rcnn_inference), roi_heads.py:1048-1091 (mask_rcnn_inference),
meta_arch/rcnn.py:242-256 (_postprocess: Detectron2's detector_postprocess with paste_masks_in_image) and
cad/evaluation/coco_evaluation.py:163-181, 398-457 (process, instances_to_coco_json).

  fast_rcnn_inference / select_detections   threshold, class-aware NMS and top-k for a whole batch: three launches, one table upload
  paste_masks                               the M x M mask logits pasted into frames (the unfused form, for tests and callers that want frames)
  coco_records                              scale to the original frame, clip, drop empty boxes, XYWH, and each mask as a COCO run-length
                                            string straight from the logits -- the frame is never written (csrc/det_post.hip, rle_stream.h)

Out of scope, on purpose:
  * averaging the cascade's stage scores (custom_cascade_rcnn.py:238-246): three softmaxes and two adds on [R, 2]; they stay torch ops
    in the caller, which hands the averaged `scores` and the last stage's `boxes` to fast_rcnn_inference;
  * the heads themselves (the RPN's proposal step is unmore_amd.rpn, the pooler between them unmore_amd.roi_pool);
  * keypoints (`pred_keypoints` in instances_to_coco_json);
  * the soft-mask variant of paste_masks_in_image (mask_threshold < 0): masks are binary, threshold in [0.5, 1].

No CPU fallback: tests/det_post_common.py restates the method in NumPy float32 (csrc/det_post.hip writes the arithmetic out)."""
import math

import numpy as np
import torch

from . import _lib as L
from . import _tables as T
from . import rle as R
from .ops import _p, _stream

MAX_CANDIDATES = 8192        # (row, class) pairs per image (csrc/det_post.hip: DP_MAX_CAND)
MAX_M = 128                  # mask side (DP_MAX_M)


def _device(tensors, what):
    return T.one_device(tensors, "det_post", what)


def _number(v, name):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"det_post: {name} must be a number, got {v!r}") from None
    if math.isnan(v):
        raise ValueError(f"det_post: {name} is NaN")
    return v


def _select_args(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image):
    boxes, scores, shapes = list(boxes), list(scores), list(image_shapes)
    if not boxes or len(boxes) != len(scores) or len(boxes) != len(shapes):
        raise ValueError(f"det_post: one boxes, scores and (h, w) entry per image and at least one image, got {len(boxes)}, {len(scores)}, "
                         f"{len(shapes)}")
    K = BC = None
    for k, (b, s) in enumerate(zip(boxes, scores)):
        for t, name in ((b, "boxes"), (s, "scores")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
                raise ValueError(f"det_post: {name}[{k}] must be a float32 matrix, got {getattr(t, 'dtype', type(t))} "
                                 f"{list(getattr(t, 'shape', []))}")
        if s.shape[1] < 2 or (K is not None and s.shape[1] != K + 1):
            raise ValueError(f"det_post: scores[{k}] has {int(s.shape[1])} columns; K + 1 >= 2 (background last), the same for every image")
        K = int(s.shape[1]) - 1
        if b.shape[1] not in (4, 4 * K) or (BC is not None and b.shape[1] != 4 * BC):
            raise ValueError(f"det_post: boxes[{k}] has {int(b.shape[1])} columns; 4 (class-agnostic) or {4 * K}, the same for every image")
        BC = int(b.shape[1]) // 4
        if b.shape[0] != s.shape[0]:
            raise ValueError(f"det_post: image {k} has {int(b.shape[0])} rows of boxes and {int(s.shape[0])} of scores")
        if int(b.shape[0]) * K > MAX_CANDIDATES:
            raise ValueError(f"det_post: image {k} has {int(b.shape[0])} rows x {K} classes = {int(b.shape[0]) * K} (row, class) pairs; "
                             f"at most {MAX_CANDIDATES} per image")
    sizes = []
    for k, s in enumerate(shapes):
        try:
            h, w = (float(v) for v in s)
        except (TypeError, ValueError):
            raise ValueError(f"det_post: image_shapes[{k}] must be (h, w), got {s!r}") from None
        if not (math.isfinite(h) and math.isfinite(w) and h >= 0 and w >= 0):
            raise ValueError(f"det_post: image_shapes[{k}] must be finite and non-negative, got {s!r}")
        sizes.append((h, w))
    st, nt = _number(score_thresh, "score_thresh"), _number(nms_thresh, "nms_thresh")
    if isinstance(topk_per_image, bool) or not isinstance(topk_per_image, (int, np.integer)):
        raise ValueError(f"det_post: topk_per_image must be an integer (negative: keep all), got {topk_per_image!r}")
    return boxes, scores, sizes, K, BC, st, nt, int(topk_per_image)


def select_detections(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image, *, _phase_ms=None):
    """The layer below fast_rcnn_inference: the same arguments, the result left on the device and nothing read back.

    Returns a dict of `pred_boxes` float32 [S, 4], `scores` float32 [S], `pred_classes` int64 [S], `rows` int64 [S] (the input row of
    each detection), `counts` int32 [N] and the Python list `first` [N]: image k's detections are the rows first[k] ... first[k] +
    counts[k] of the four tensors, in descending score order; its slot holds min(R_k * K, topk) rows (R_k * K when topk < 0), the rows
    past counts[k] are undefined.  Three launches and the blocking upload of the table of images."""
    boxes, scores, sizes, K, BC, st, nt, topk = _select_args(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image)
    dev = _device(boxes + scores, "select_detections")
    N = len(boxes)
    tab = (L.DpImage * N)()
    hold, first = [], []
    cand = out = words = max_cand = 0
    for k, (b, s, (h, w)) in enumerate(zip(boxes, scores, sizes)):
        b, s = b.detach().contiguous(), s.detach().contiguous()
        hold += [b, s]
        P = int(b.shape[0]) * K
        e = tab[k]
        e.boxes, e.scores = (b.data_ptr(), s.data_ptr()) if P else (None, None)
        e.mat_first, e.R, e.cand_first, e.out_first = words, int(b.shape[0]), cand, out
        e.cap = P if topk < 0 else min(P, topk)
        e.height, e.width = h, w
        first.append(out)
        cand, out, words, max_cand = cand + P, out + e.cap, words + P * ((P + 63) // 64), max(max_cand, P)
    with torch.cuda.device(dev):
        res = {"pred_boxes": torch.empty((out, 4), dtype=torch.float32, device=dev), "scores": torch.empty(out, dtype=torch.float32, device=dev),
               "pred_classes": torch.empty(out, dtype=torch.int64, device=dev), "rows": torch.empty(out, dtype=torch.int64, device=dev),
               "counts": torch.empty(N, dtype=torch.int32, device=dev), "first": first}
        buf = T.upload(tab, N, dev)[0]
        nbytes = L.lib().umr_det_select_workspace(N, cand, words)
        ws = T.workspace(nbytes, dev)

        def launch(phases):
            L.check(L.lib().umr_det_select(_p(buf), N, K, BC, cand, max_cand, words, out, st, nt, max(topk, -1), phases, _p(res["pred_boxes"]),
                                           _p(res["scores"]), _p(res["pred_classes"]), _p(res["rows"]), _p(res["counts"]), _p(ws), nbytes,
                                           _stream()), "umr_det_select")
        T.timed(launch, (("candidates", 1), ("suppression", 2), ("scan", 4)), _phase_ms)       # tools/detector_post_bench.py times the launches
        del hold
    return res


def split_detections(selected):
    """the per-image views of select_detections' result; reads `counts` (one synchronisation): (items, kept rows)"""
    counts = [int(v) for v in selected["counts"].tolist()]
    items, rows = [], []
    for f, n in zip(selected["first"], counts):
        items.append({"pred_boxes": selected["pred_boxes"][f:f + n], "scores": selected["scores"][f:f + n],
                      "pred_classes": selected["pred_classes"][f:f + n]})
        rows.append(selected["rows"][f:f + n])
    return items, rows


def fast_rcnn_inference(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image):
    """The reference's fast_rcnn_inference (fast_rcnn.py:52-179) for the whole batch in one call: a fixed number of launches and one
    read of the kept counts.

    boxes[i]: float32 [R_i, 4] (class-agnostic, the recipe) or [R_i, K * 4]; scores[i]: float32 [R_i, K + 1], probabilities with the
    background column last; image_shapes[i]: (h, w) -- what Boxes.clip reads; the reference's docstring says (width, height) and is
    wrong.  Returns (items, kept_indices): per image a dict with `pred_boxes` float32 [n_i, 4], `scores` float32 [n_i] and
    `pred_classes` int64 [n_i] (views into the batch's buffers), and the kept row indices int64 [n_i].

    In the reference's order: a row with a non-finite box or score entry is dropped; the last score column is dropped; boxes are
    clipped to (h, w); the candidates are the (row, class) pairs with score > score_thresh, strictly, in nonzero() order; greedy NMS
    per class in descending score order, equal scores in candidate order (what umr_nms defines and torchvision's stable CPU sort
    gives): a candidate goes iff an earlier kept one of its class has inter / ((area_a + area_b) - inter) > nms_thresh, float32 with
    every operation rounded on its own, so that the kept set equals a float32 NumPy restatement exactly (0 / 0 is NaN and suppresses
    nothing); the kept ones in descending score order across classes, the first topk_per_image when that is >= 0.

    A documented departure: this is torchvision's _batched_nms_vanilla, NMS per class on the boxes as they are.  Detectron2's batched_nms
    reaches torchvision's coordinate trick for small inputs, which adds class * (max_coordinate + 1) to every box.  With one class
    (the recipe) the offset is zero and the two rules agree bit for bit; with more classes the shifted boxes round differently and a
    pair whose IoU lies within rounding of the threshold can fall on the other side.

    At most 8192 (row, class) pairs per image (ValueError before any launch).  Every argument error is a ValueError before any
    launch; CPU tensors raise RuntimeError.  No float atomics: the same input gives the same bytes."""
    return split_detections(select_detections(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image))


# ---------------------------------------------------------------------------------------------------------------- the mask side
def _check_logits(mask_logits, n):
    m = mask_logits
    if not isinstance(m, torch.Tensor) or m.dtype not in (torch.float32, torch.bfloat16) or m.dim() != 4 or m.shape[2] != m.shape[3]:
        raise ValueError(f"det_post: mask_logits must be float32 or bfloat16 [N, C, M, M], got {getattr(m, 'dtype', type(m))} "
                         f"{list(getattr(m, 'shape', []))}")
    if m.shape[0] != n:
        raise ValueError(f"det_post: {int(m.shape[0])} masks for {n} boxes")
    if m.shape[1] < 1 or not 1 <= m.shape[2] <= MAX_M:
        raise ValueError(f"det_post: mask_logits needs C >= 1 and 1 <= M <= {MAX_M}, got {list(m.shape)}")
    return int(m.shape[1]), int(m.shape[2])


def _check_threshold(threshold):
    t = _number(threshold, "threshold")
    if not 0.5 <= t <= 1.0:
        raise ValueError(f"det_post: the mask threshold must lie in [0.5, 1] (the soft-mask variant is out of scope), got {threshold!r}")
    return t


def _check_frame(h, w, what):
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, (int, np.integer)) or not isinstance(w, (int, np.integer)) \
            or h <= 0 or w <= 0 or int(h) * int(w) >= 1 << 31:
        raise ValueError(f"det_post: {what} must be positive integers (height, width) with height * width < 2^31, got {(h, w)!r}")
    return int(h), int(w)


def _check_rows(boxes, classes, what):
    boxes = T.unwrap(boxes)
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError(f"det_post: {what}: boxes must be float32 [n, 4], got {getattr(boxes, 'dtype', type(boxes))} "
                         f"{list(getattr(boxes, 'shape', []))}")
    n = int(boxes.shape[0])
    if classes is not None and (not isinstance(classes, torch.Tensor) or classes.dtype != torch.int64 or tuple(classes.shape) != (n,)):
        raise ValueError(f"det_post: {what}: pred_classes must be int64 [{n}], got {getattr(classes, 'dtype', type(classes))} "
                         f"{list(getattr(classes, 'shape', []))}")
    return boxes, n


def paste_masks(mask_logits, boxes, pred_classes, height, width, threshold=0.5):
    """Detectron2's paste_masks_in_image after mask_rcnn_inference, for one image: uint8 [N, height, width] of 0 / 1, on the device.

    mask_logits: float32 or bfloat16 [N, C, M, M]; C == 1 is class-agnostic, otherwise channel pred_classes[n] (int64 [N]; a class
    without a channel gives an empty mask) is used.  boxes: float32 [N, 4] XYXY in the frame.  The probability is sigmoid(logit) in
    float32; pixel (y, x) is set iff the bilinear sample of F.grid_sample(align_corners=False, zero padding) at the pixel's centre is
    >= threshold.  csrc/det_post.hip writes the float32 operation order out and evaluates only the rows and columns of the box,
    rounded outward and clipped to the frame: a pixel whose centre lies outside the box has a weight below 1/2 and so a value below
    1/2, which is why threshold must lie in [0.5, 1].  A box that is not finite or has no positive width and height sets nothing.
    One launch (and the memset of the frames), nothing read back."""
    boxes, n = _check_rows(boxes, pred_classes, "paste_masks")
    C, M = _check_logits(mask_logits, n)
    if C > 1 and pred_classes is None:
        raise ValueError("det_post: paste_masks: class-specific mask_logits need pred_classes")
    H, W = _check_frame(height, width, "the frame")
    t = _check_threshold(threshold)
    dev = _device([mask_logits, boxes] + ([pred_classes] if pred_classes is not None else []), "paste_masks")
    with torch.cuda.device(dev):
        out = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
        if n:
            m, b = mask_logits.detach().contiguous(), boxes.detach().contiguous()
            c = None if pred_classes is None else pred_classes.contiguous()
            L.check(L.lib().umr_det_paste(_p(m), T.dtype_code(m), n, C, M, _p(c), _p(b), 4, H, W, t, _p(out), _stream()), "umr_det_paste")
    return out


def scale_ratio(out_size, in_size):
    """the float32 factor detector_postprocess hands Boxes.scale: the Python double ratio, rounded to float32 as a float32 tensor's
    in-place multiplication by a Python number does"""
    return float(np.float32(float(out_size) / float(in_size)))


def coco_records(detections, mask_logits, image_sizes, output_sizes, image_ids, category_ids=None, threshold=0.5, *, _phase_ms=None):
    """What detector_postprocess and instances_to_coco_json make of a batch's detections: one list of COCO result records per image.

    detections: what fast_rcnn_inference returns -- per image a dict (or an object) with `pred_boxes` float32 [n_i, 4], `scores`
    float32 [n_i] and `pred_classes` int64 [n_i], in the network's input frame.  mask_logits: float32 or bfloat16 [sum n_i, C, M, M] in
    image order (C == 1: class-agnostic; else the predicted class's channel), or None: records without `segmentation`.  image_sizes:
    the network's input (h, w) per image; output_sizes: the original frame's (height, width) per image, positive integers;
    category_ids: maps the class index to the dataset's category id (a dict or a sequence), identity when None.

    Per image: the boxes are scaled by float32(out_w / in_w) and float32(out_h / in_h) (the Python double ratio rounded to float32
    first), clipped to the output size, rows with width <= 0 or height <= 0 are dropped; a record is {"image_id", "category_id",
    "bbox": [x0, y0, fl32(x1 - x0), fl32(y1 - y0)], "score", "segmentation": {"size": [H, W], "counts": str}} in that order, all numbers
    Python floats / ints.  The mask is paste_masks' mask of the scaled box in the output frame, never written: a producer for
    rle_stream.h evaluates the paste over the box's columns in column-major order and the strings come out of the measure pass and the
    packed write pass of rle._two_pass, every mask in its own image's size, all images in one pair of launches.  Host reads: the scaled
    boxes with the scores, the classes, the string sizes, the characters.  Images without detections give []."""
    detections, in_sizes, out_sizes, image_ids = list(detections), list(image_sizes), list(output_sizes), list(image_ids)
    N = len(detections)
    if not N or len(in_sizes) != N or len(out_sizes) != N or len(image_ids) != N:
        raise ValueError(f"det_post: coco_records needs one image size, output size and image id per image and at least one image, got "
                         f"{N}, {len(in_sizes)}, {len(out_sizes)}, {len(image_ids)}")
    boxes, scores, classes, counts, rowinfo = [], [], [], [], []
    for k, d in enumerate(detections):
        get = T.getter(d)
        c, s = get("pred_classes"), get("scores")
        b, _ = _check_rows(get("pred_boxes"), c, f"detections[{k}]")
        if c is None or not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or tuple(s.shape) != (len(b),):
            raise ValueError(f"det_post: detections[{k}] needs scores float32 [{len(b)}] and pred_classes int64 [{len(b)}]")
        try:
            ih, iw = (float(v) for v in in_sizes[k])
            oh, ow = out_sizes[k]
        except (TypeError, ValueError):
            raise ValueError(f"det_post: image {k}: sizes are (h, w) pairs") from None
        if not (math.isfinite(ih) and math.isfinite(iw) and ih > 0 and iw > 0):
            raise ValueError(f"det_post: image_sizes[{k}] must be positive and finite, got {in_sizes[k]!r}")
        oh, ow = _check_frame(oh, ow, f"output_sizes[{k}]")
        boxes.append(b), scores.append(s), classes.append(c), counts.append(len(b))
        info = np.zeros((len(b), 4), dtype=np.float32)
        info[:, 0], info[:, 1] = scale_ratio(ow, iw), scale_ratio(oh, ih)
        info.view(np.int32)[:, 2], info.view(np.int32)[:, 3] = oh, ow
        rowinfo.append(info)
    n = sum(counts)
    t = _check_threshold(threshold)
    tensors = boxes + scores + classes
    if mask_logits is not None:
        C, M = _check_logits(mask_logits, n)
        tensors = tensors + [mask_logits]
    dev = _device(tensors, "coco_records")
    if category_ids is not None and not isinstance(category_ids, dict):
        category_ids = dict(enumerate(category_ids))
    if n == 0:
        return [[] for _ in range(N)]
    with torch.cuda.device(dev):
        b_all, s_all, c_all = torch.cat(boxes).contiguous(), torch.cat(scores), torch.cat(classes).contiguous()
        info = torch.from_numpy(np.concatenate(rowinfo)).to(dev)
        rec = torch.empty((n, 8), dtype=torch.float32, device=dev)
        L.check(L.lib().umr_det_scale(_p(b_all), _p(info), n, _p(rec), _stream()), "umr_det_scale")
        rec[:, 7] = s_all
        strings = None
        if mask_logits is not None:
            m = mask_logits.detach().contiguous()
            frames = info.view(torch.int32)[:, 2:]                                   # (H, W) per mask, stride 4

            def run(sizes, offsets, chars, cap):
                L.check(L.lib().umr_det_paste_rle(_p(m), T.dtype_code(m), n, C, M, _p(c_all), _p(rec), 8, _p(frames), 4, t,
                                                  _p(sizes), _p(offsets), _p(chars), cap, _stream()), "umr_det_paste_rle")

            def launch(sizes, offsets, chars, cap):
                T.timed(lambda _: run(sizes, offsets, chars, cap), (("write" if chars is not None else "measure", 1),), _phase_ms)
            strings = R._two_pass(launch, n, 0, 0, dev)
        host = rec.cpu().numpy()
        cls = c_all.cpu().tolist()
    out, at = [], 0
    for k in range(N):
        mine = []
        oh, ow = int(out_sizes[k][0]), int(out_sizes[k][1])
        for i in range(at, at + counts[k]):
            if host[i, 6] == 0:
                continue
            r = {"image_id": image_ids[k], "category_id": cls[i] if category_ids is None else category_ids[cls[i]],
                 "bbox": [float(host[i, 0]), float(host[i, 1]), float(host[i, 4]), float(host[i, 5])], "score": float(host[i, 7])}
            if strings is not None:
                r["segmentation"] = {"size": [oh, ow], "counts": strings[i]["counts"]}
            mine.append(r)
        out.append(mine)
        at += counts[k]
    return out
