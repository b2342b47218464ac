"""Generate tests/golden/det_post.npz by running the REFERENCE's own inference tail on the CPU.

Run where the reference tree is at hand, never on the GPU box:
    python tests/golden/make_golden_det_post.py /path/to/reference

What executes verbatim from the reference, read at generation time and compiled in a namespace of stand-ins; none of it is stored here:
  cad/modeling/roi_heads/fast_rcnn.py              fast_rcnn_inference, fast_rcnn_inference_single_image, and FastRCNNOutputLayers.predict_boxes
                                                   / predict_probs
  cad/modeling/roi_heads/custom_cascade_rcnn.py    CustomCascadeROIHeads._forward_box (its inference branch) and _create_proposals_from_boxes
  cad/modeling/roi_heads/roi_heads.py              mask_rcnn_inference
  cad/evaluation/coco_evaluation.py                instances_to_coco_json
The functions are cut out one by one (make_golden_box_loss.cut) because their files import Detectron2, fvcore and pycocotools, which are
absent.  _forward_box runs with a stand-in `self`: three stages, `_run_stage` returns predictions drawn here from a seeded generator,
`box_predictor[k]` carries the recipe's settings (one class, class-agnostic regression, SCORE_THRESH_TEST 0.0, NMS_THRESH_TEST 0.5,
DETECTIONS_PER_IMAGE 100 -- cut to 12 here so that the top-k cut is exercised) and the two cut-out methods.

The stand-ins written here from Detectron2's and torchvision's published definitions, and so the semantics that rest on them and not on
the reference: `Boxes` (tensor, len, indexing, clip, scale, nonempty), `Instances` (fields, has, get_fields, indexing, image_size),
`batched_nms` (Detectron2's: float32 boxes to torchvision.ops.batched_nms, which for fewer than 4000 boxes is the coordinate trick:
offsets class * (max coordinate + 1), then nms) with `nms` (torchvision's CPU kernel: descending STABLE sort of the scores, areas
(x2 - x1) * (y2 - y1), inter / (area_i + area_j - inter) > threshold, in float32), `Box2BoxTransform` (make_golden_box_loss's),
`BoxMode.convert` (XYXY_ABS -> XYWH_ABS: columns 2 and 3 minus columns 0 and 1, in the array's float32), `detector_postprocess`
(scale by (out_w / in_w, out_h / in_h), clip, keep nonempty, paste with threshold 0.5), `paste_masks_in_image` (_do_paste_mask with
torch CPU F.grid_sample in float32, then >= 0.5: det_post_common.paste_torch), `mask_util.encode` (the repository's rle.encode_numpy,
counts as bytes), `cat` and `move_device_like`.

Batch: five images (network frames up to 96 x 130, output frames at ratios 2x exactly, non-integer, 1x, and two more), 40-90 proposals
each, one image whose proposals include boxes that become empty after scale and clip.  Stored: the reference's averaged `scores` and
last-stage `boxes` (the inputs of fast_rcnn_inference), the thresholds, the mask logits, and as expected outputs the instances, the
kept indices and the records with their masks as run-length strings.  The generator asserts that no two candidates of an image have
the same score (torch's unstable final sort would leave their order open) and that the reference's own float32 paste stays under the
band rule's cap against float64.  float32 torch on the CPU.  Only arrays are stored."""
import os
import sys
from typing import List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import det_post_common as C  # noqa: E402
from make_golden_box_loss import Bag, Box2BoxTransform, bind, cat, cut  # noqa: E402
from unmore_amd import rle  # noqa: E402

IN_SIZES = [(48, 65), (50, 67), (96, 130), (60, 80), (72, 100)]
OUT_SIZES = [(96, 130), (37, 53), (96, 130), (45, 60), (100, 130)]
PROPOSALS = [60, 40, 90, 50, 70]
WEIGHTS = [(10., 10., 5., 5.), (20., 20., 10., 10.), (30., 30., 15., 15.)]
SCORE_THRESH, NMS_THRESH, TOPK, M = 0.0, 0.5, 12, 28


# ---------------------------------------------------------------------------------------------------------------- stand-ins
class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor.reshape(-1, 4).to(torch.float32)

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, item):
        return Boxes(self.tensor[item].reshape(-1, 4))

    def clip(self, box_size):
        h, w = box_size
        x1, y1 = self.tensor[:, 0].clamp(min=0, max=w), self.tensor[:, 1].clamp(min=0, max=h)
        x2, y2 = self.tensor[:, 2].clamp(min=0, max=w), self.tensor[:, 3].clamp(min=0, max=h)
        self.tensor = torch.stack((x1, y1, x2, y2), dim=-1)

    def scale(self, scale_x, scale_y):
        self.tensor[:, 0::2] *= scale_x
        self.tensor[:, 1::2] *= scale_y

    def nonempty(self, threshold=0.0):
        b = self.tensor
        return ((b[:, 2] - b[:, 0]) > threshold) & ((b[:, 3] - b[:, 1]) > threshold)


class Instances:
    def __init__(self, image_size, **fields):
        object.__setattr__(self, "_fields", dict(fields))
        object.__setattr__(self, "image_size", image_size)

    def __setattr__(self, name, value):
        self._fields[name] = value

    def __getattr__(self, name):
        fields = object.__getattribute__(self, "_fields")
        if name not in fields:
            raise AttributeError(name)
        return fields[name]

    def has(self, name):
        return name in self._fields

    def get_fields(self):
        return self._fields

    def __getitem__(self, item):
        return Instances(self.image_size, **{k: v[item] for k, v in self._fields.items()})

    def __len__(self):
        for v in self._fields.values():
            return len(v)
        return 0


def nms(boxes, scores, iou_threshold):
    """torchvision's CPU nms kernel, float32"""
    b = boxes.numpy().astype(np.float32)
    order = torch.sort(scores, stable=True, descending=True).indices.numpy()
    areas = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32)
    suppressed = np.zeros(len(b), bool)
    keep = []
    thr = np.float32(iou_threshold)
    for _i in range(len(b)):
        i = order[_i]
        if suppressed[i]:
            continue
        keep.append(i)
        for _j in range(_i + 1, len(b)):
            j = order[_j]
            if suppressed[j]:
                continue
            xx1, yy1 = max(b[i, 0], b[j, 0]), max(b[i, 1], b[j, 1])
            xx2, yy2 = min(b[i, 2], b[j, 2]), min(b[i, 3], b[j, 3])
            w, h = max(np.float32(0), np.float32(xx2 - xx1)), max(np.float32(0), np.float32(yy2 - yy1))
            inter = np.float32(w * h)
            with np.errstate(invalid="ignore", divide="ignore"):
                ovr = np.float32(inter / np.float32(np.float32(areas[i] + areas[j]) - inter))
            if ovr > thr:
                suppressed[j] = True
    return torch.as_tensor(np.array(keep, dtype=np.int64))


def batched_nms(boxes, scores, idxs, iou_threshold):
    """Detectron2's batched_nms -> torchvision.ops.batched_nms, the coordinate trick (fewer than 4000 boxes)"""
    assert boxes.shape[-1] == 4
    boxes = boxes.float()
    if boxes.numel() == 0:
        return torch.empty((0,), dtype=torch.int64)
    max_coordinate = boxes.max()
    offsets = idxs.to(boxes) * (max_coordinate + torch.tensor(1).to(boxes))
    return nms(boxes + offsets[:, None], scores, iou_threshold)


class BoxMode:
    XYXY_ABS, XYWH_ABS = 0, 1

    @staticmethod
    def convert(box, from_mode, to_mode):
        assert (from_mode, to_mode) == (BoxMode.XYXY_ABS, BoxMode.XYWH_ABS)
        arr = torch.from_numpy(np.asarray(box)).clone()
        arr[:, 2] -= arr[:, 0]
        arr[:, 3] -= arr[:, 1]
        return arr.numpy()


def paste_masks_in_image(masks, boxes, image_shape, threshold=0.5):
    h, w = image_shape
    if len(masks) == 0:
        return torch.zeros((0, h, w), dtype=torch.bool)
    return torch.from_numpy(C.paste_torch(masks.numpy(), boxes.tensor.numpy(), h, w) >= threshold)


def detector_postprocess(results, output_height, output_width, mask_threshold=0.5):
    scale_x, scale_y = output_width / results.image_size[1], output_height / results.image_size[0]
    results = Instances((output_height, output_width), **results.get_fields())
    output_boxes = results.pred_boxes
    output_boxes.scale(scale_x, scale_y)
    output_boxes.clip(results.image_size)
    results = results[output_boxes.nonempty()]
    if results.has("pred_masks"):
        results.pred_masks = paste_masks_in_image(results.pred_masks[:, 0, :, :], results.pred_boxes, (output_height, output_width), mask_threshold)
    return results


class mask_util:
    @staticmethod
    def encode(arr):
        assert arr.ndim == 3 and arr.flags["F_CONTIGUOUS"] and arr.dtype == np.uint8
        out = []
        for k in range(arr.shape[2]):
            r = rle.encode_numpy(arr[:, :, k])
            out.append({"size": r["size"], "counts": r["counts"].encode("ascii")})
        return out


def load_reference(ref):
    ns = {"torch": torch, "F": F, "np": np, "List": List, "Tuple": Tuple, "Boxes": Boxes, "Instances": Instances, "cat": cat,
          "batched_nms": batched_nms, "BoxMode": BoxMode, "mask_util": mask_util, "move_device_like": lambda src, dst: src.to(dst.device)}
    fast = os.path.join(ref, "cad", "modeling", "roi_heads", "fast_rcnn.py")
    for name in ("fast_rcnn_inference", "fast_rcnn_inference_single_image"):
        exec(cut(fast, name), ns)
    for name in ("predict_boxes", "predict_probs"):
        exec(cut(fast, name, "    "), ns)
    cascade = os.path.join(ref, "cad", "modeling", "roi_heads", "custom_cascade_rcnn.py")
    for name in ("_forward_box", "_create_proposals_from_boxes"):
        exec(cut(cascade, name, "    "), ns)
    exec(cut(os.path.join(ref, "cad", "modeling", "roi_heads", "roi_heads.py"), "mask_rcnn_inference"), ns)
    exec(cut(os.path.join(ref, "cad", "evaluation", "coco_evaluation.py"), "instances_to_coco_json"), ns)
    return ns


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ns = load_reference(sys.argv[1])
    rng = np.random.RandomState(57)
    N = len(IN_SIZES)
    proposals = []
    for (h, w), n in zip(IN_SIZES, PROPOSALS):
        centres = rng.uniform(0.2, 0.8, (6, 2)) * [w, h]                       # six objects, the proposals scatter around them
        which = rng.randint(6, size=n)
        c = centres[which] + rng.normal(0, 2.0, (n, 2))
        s = rng.uniform(0.18, 0.4, (n, 2)) * [w, h]
        p = np.concatenate([c - s / 2, c + s / 2], axis=1).astype(np.float32)
        proposals.append(Instances((h, w), proposal_boxes=Boxes(torch.from_numpy(p))))
    far = proposals[1].proposal_boxes.tensor
    far[3] = torch.tensor([200., 10., 230., 30.])                              # outside the frame: clips to zero width, dropped by the postprocess

    captured = {}
    real = ns["fast_rcnn_inference"]

    def fast_rcnn_inference(boxes, scores, image_shapes, score_thresh, nms_thresh, topk):
        captured.update(boxes=[b.clone() for b in boxes], scores=[s.clone() for s in scores], shapes=list(image_shapes))
        out = real(boxes, scores, image_shapes, score_thresh, nms_thresh, topk)
        captured["kept"] = out[1]
        return out
    ns["fast_rcnn_inference"] = fast_rcnn_inference

    def predictor(k):
        p = Bag(box2box_transform=Box2BoxTransform(WEIGHTS[k]), use_sigmoid_ce=False, test_score_thresh=SCORE_THRESH,
                test_nms_thresh=NMS_THRESH, test_topk_per_image=TOPK)
        bind(p, ns, "predict_boxes", "predict_probs")
        return p

    def run_stage(features, props, k):
        R = sum(len(p) for p in props)
        scores = torch.from_numpy((rng.standard_normal((R, 2)) * 1.5).astype(np.float32))
        scores[PROPOSALS[0] + 3] = torch.tensor([6., -6.])                     # the far box of image 1 scores high in every stage: it is kept
        deltas = torch.from_numpy((rng.standard_normal((R, 4)) * 0.03).astype(np.float32) * np.array(WEIGHTS[k], dtype=np.float32))
        return scores, deltas

    heads = Bag(box_in_features=[], num_cascade_stages=3, training=False, box_predictor=[predictor(k) for k in range(3)], _run_stage=run_stage)
    bind(heads, ns, "_forward_box", "_create_proposals_from_boxes")
    with torch.no_grad():
        instances = heads._forward_box({}, proposals)
    counts = [len(x) for x in instances]
    assert max(counts) == TOPK and min(counts) > 0, counts
    for s in captured["scores"]:                                               # no exact ties among the candidates
        v = s[:, 0].numpy()
        assert len(np.unique(v)) == len(v), "two candidates share a score"

    logits = torch.from_numpy(C.smooth_logits(rng, sum(counts), 1, M))
    ns["mask_rcnn_inference"](logits, instances)
    arrays = {"n_images": np.int64(N), "in_sizes": np.array(IN_SIZES, dtype=np.int64), "out_sizes": np.array(OUT_SIZES, dtype=np.int64),
              "score_thresh": np.float64(SCORE_THRESH), "nms_thresh": np.float64(NMS_THRESH), "topk": np.int64(TOPK),
              "mask_logits": logits.numpy()}
    n_band = n_pos = 0
    for k in range(N):
        arrays[f"im{k}_boxes"], arrays[f"im{k}_scores"] = captured["boxes"][k].numpy(), captured["scores"][k].numpy()
        arrays[f"im{k}_pred_boxes"] = instances[k].pred_boxes.tensor.numpy().copy()
        arrays[f"im{k}_pred_scores"], arrays[f"im{k}_pred_classes"] = instances[k].scores.numpy(), instances[k].pred_classes.numpy()
        arrays[f"im{k}_kept"] = captured["kept"][k].numpy()
        probs = instances[k].pred_masks[:, 0].numpy()
        post = detector_postprocess(instances[k], *OUT_SIZES[k])
        recs = ns["instances_to_coco_json"](post.to("cpu") if hasattr(post, "to") else post, 100 + k)
        arrays[f"im{k}_rec_n"] = np.int64(len(recs))
        arrays[f"im{k}_rec_bbox"] = np.array([r["bbox"] for r in recs], dtype=np.float64).reshape(-1, 4)
        arrays[f"im{k}_rec_score"] = np.array([r["score"] for r in recs], dtype=np.float64)
        arrays[f"im{k}_rec_category"] = np.array([r["category_id"] for r in recs], dtype=np.int64)
        arrays[f"im{k}_rec_counts"] = np.array([r["segmentation"]["counts"] for r in recs], dtype="S")
        assert all(list(r) == ["image_id", "category_id", "bbox", "score", "segmentation"] and r["segmentation"]["size"] == list(OUT_SIZES[k])
                   for r in recs)
        # the reference's own float32 paste against float64, by the band rule
        b, keep = C.postprocess_numpy(arrays[f"im{k}_pred_boxes"], IN_SIZES[k], OUT_SIZES[k])
        assert int(keep.sum()) == len(recs)
        got = np.stack([rle.decode_numpy({"size": list(OUT_SIZES[k]), "counts": r["segmentation"]["counts"]}) for r in recs])
        n_band += C.band_check(got, probs[keep], b[keep], *OUT_SIZES[k], what=f"reference, image {k}")
        print(f"image {k}: {PROPOSALS[k]} proposals, {counts[k]} kept, {len(recs)} records")
    assert arrays["im1_rec_n"] < counts[1], "no box became empty in the postprocess"
    path = os.path.join(HERE, "det_post.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size} bytes)")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()
