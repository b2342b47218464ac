"""Host-side mirror of the reference's `Object_Scoring` (object_scoring.py:43-272) -- the second caller of the ObjectnessNet hot path at
inference: for the boxes object discovery found in an image, predict both fields and the existence score on their 128 x 128 crops, turn
the fields into a mask per box, tighten the box to its mask, NMS, score what is left and write one record per survivor -- with its mask
as a COCO run-length string -- to `object_discovery_with_scores.json`.  What is NOT mirrored: the COCO dataset object and the reading of
the raw-annotation JSON (`main_object_scoring` takes the images and the boxes).

The reference builds, per proposal, two image-sized int64 canvases in a Python loop (Resize of the crop-sized mask into the box, paste),
stacks them ([N,H,W] twice, plus their union), takes every tight box through pycocotools on the host, and only then runs NMS.  Here one
launch reduces each proposal's pasted union mask to its tight box, its area and the two field maxima without writing anything
image-sized (csrc/reasoning.hip::mask_paste_stats_kernel); NMS runs on those; the masks are materialised for the survivors only -- or
not at all: the reference walks every survivor's mask through pycocotools on the host for its `segmentation` string (:166-170,262);
here csrc/rle.hip::mask_paste_rle_kernel encodes the pasted mask straight from the two crop masks in LDS (`score_image(segmentation=
True)`), and with `masks=False` the strings, about 300 times smaller than the masks, are all that is made."""

import json

import numpy as np
import torch

from . import _lib as L
from . import reasoning
from . import rle
from .ops import _p, _stream


class _NumpyEncoder(json.JSONEncoder):
    """what the reference's utils/misc.py::NpEncoder does for the values a record holds: numpy integers, floats and booleans become
    Python's, arrays become lists"""
    def default(self, o):
        if isinstance(o, np.integer):
            return int(o)
        if isinstance(o, np.floating):
            return float(o)
        if isinstance(o, np.bool_):
            return bool(o)
        if isinstance(o, np.ndarray):
            return o.tolist()
        return super().default(o)


def write_annotations(records, path):
    """object_scoring.py:271-272: the record list as JSON, indent=2"""
    with open(path, "w") as f:
        json.dump(records, f, indent=2, cls=_NumpyEncoder)


class Object_Scoring:
    def __init__(self, args, device, objectness_model=None, binary_classifier_model=None):
        """object_scoring.py:45-104: both networks restored from `args.objectness_resume` / `args.binary_classifier_resume` (:59-90)
        unless they are handed in; fp32, eval, frozen."""
        self.args, self.device = args, torch.device(device)
        if objectness_model is None:
            from .objectness_net import ObjectnessNet
            objectness_model = ObjectnessNet(device=self.device, image_size=args.image_size, backbone_type=args.backbone_type, args=args).to(self.device)
            objectness_model.load_state_dict(torch.load(args.objectness_resume, map_location=self.device)["model_state_dict"], strict=True)
            objectness_model = objectness_model.to(torch.float32)
        if binary_classifier_model is None:
            from .binary_classifier import Binary_Classifier
            binary_classifier_model = Binary_Classifier(device=self.device, image_size=args.image_size, args=args).to(self.device)
            binary_classifier_model.load_state_dict(torch.load(args.binary_classifier_resume, map_location=self.device)["model_state_dict"], strict=True)
            binary_classifier_model = binary_classifier_model.to(torch.float32)
        self.objectness_model, self.binary_classifier_model = objectness_model, binary_classifier_model
        for m in (objectness_model, binary_classifier_model):
            if isinstance(m, torch.nn.Module):
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def get_prediction_with_proposals(self, image, proposals):
        """object_scoring.py:112-157: {'pred_boundary_fields' [N,128,128], 'pred_center_fields' [N,2,128,128], 'pred_existence_scores' [N]}"""
        out = reasoning.get_prediction_with_proposals(self.objectness_model, self.binary_classifier_model, image, proposals)
        return {k: out[k] for k in ("pred_boundary_fields", "pred_center_fields", "pred_existence_scores")}

    def score_image(self, image, raw_proposals, segmentation=False, masks=True):
        """object_scoring.py:182-255 for one image.  image [3,H,W] f32 (moved to the GPU), raw_proposals: N boxes [x1,y1,x2,y2].
        Returns a dict of what the reference writes per surviving box, in NMS order: 'tight_bboxes' [K,4] f32 (x1,y1,x2,y2), 'masks'
        [K,H,W] u8 on the GPU, and numpy arrays 'score' (f64), 'existence_score', 'center_score', 'boundary_score' (f32), 'area_score' (f64).
        segmentation=True adds 'segmentation': the K masks' COCO run-length records (:166-170), encoded on the device without the masks;
        masks=False leaves 'masks' None (no image-sized mask is written)."""
        image = image.to(self.device, torch.float32)
        H, W = image.shape[-2], image.shape[-1]
        props = torch.as_tensor(np.asarray(raw_proposals, dtype=np.float64)).reshape(-1, 4)
        N = len(props)
        if N == 0:
            return None
        pred = self.get_prediction_with_proposals(image, props)
        sdf = pred["pred_boundary_fields"].contiguous().float()
        cen = pred["pred_center_fields"].contiguous().float()
        S = sdf.shape[-1]
        # the box a mask is pasted into: floor / ceil corners (:200-202), clipped like the slice `canvas[y1:y2, x1:x2]` clips them
        ib = torch.stack([torch.floor(props[:, 0]), torch.floor(props[:, 1]), torch.ceil(props[:, 2]), torch.ceil(props[:, 3])], 1).to(torch.int32)
        ib[:, 0].clamp_(0, W); ib[:, 2].clamp_(0, W); ib[:, 1].clamp_(0, H); ib[:, 3].clamp_(0, H)   # noqa: E702
        ib = ib.to(self.device).contiguous()
        stats = torch.empty((N, 5), dtype=torch.int32, device=self.device)
        maxima = torch.empty((N, 2), dtype=torch.float32, device=self.device)
        L.check(L.lib().umr_mask_paste_stats(_p(sdf), _p(cen), _p(ib), N, S, H, W, _p(stats), _p(maxima), _stream()), "umr_mask_paste_stats")
        tight = stats[:, :4].to(torch.float32)                                   # torch.FloatTensor(tight_bboxes), :235
        max_center, max_boundary = maxima[:, 0], maxima[:, 1]                    # :189-193
        keep = reasoning.nms(tight, max_boundary, iou_threshold=0.5)            # :238
        K = len(keep)
        if masks:
            masks = torch.empty((K, H, W), dtype=torch.uint8, device=self.device)
            L.check(L.lib().umr_mask_paste(_p(sdf), _p(cen), _p(ib), _p(keep.contiguous()), K, S, H, W, _p(masks), _stream()), "umr_mask_paste")
        else:
            masks = None
        area = stats[:, 4][keep].cpu().numpy().astype(np.int64)                  # final_binary_masks.sum(1).sum(1), :244-245
        existence = pred["pred_existence_scores"][keep].cpu().numpy()
        center = max_center[keep].cpu().numpy()
        boundary = max_boundary[keep].cpu().numpy()
        mask_scores = area / area.max()
        area_score = np.power(mask_scores, 0.25)
        score = existence * center * boundary * area_score                      # :255
        out = {"tight_bboxes": tight[keep], "masks": masks, "score": score, "existence_score": existence, "center_score": center,
               "boundary_score": boundary, "area_score": area_score, "keep": keep}
        if segmentation:
            out["segmentation"] = rle.encode_pasted(sdf, cen, ib, keep, H, W)      # binary_mask_to_rle of every survivor, :262
        return out

    def annotations(self, image_id, scored):
        """the reference's per-box records (:257-267), keys in its order; 'segmentation' (the COCO run-length record of the box's mask)
        when `scored` has it (`score_image(segmentation=True)`)"""
        out = []
        if scored is None:
            return out
        seg = scored.get("segmentation")
        for i, (x1, y1, x2, y2) in enumerate(scored["tight_bboxes"].cpu().numpy()):
            rec = {"image_id": image_id, "category_id": 1, "score": scored["score"][i], "bbox": [x1, y1, x2 - x1, y2 - y1]}
            if seg is not None:
                rec["segmentation"] = seg[i]
            rec.update({"existence_score": scored["existence_score"][i], "center_score": scored["center_score"][i],
                        "boundary_score": scored["boundary_score"][i], "area_score": scored["area_score"][i]})
            out.append(rec)
        return out

    def main_object_scoring(self, images, raw_annotations, segmentation=False, out_path=None):
        """object_scoring.py:172-272 without the dataset object: `images` yields (image_id, image), `raw_annotations` maps str(image_id) ->
        boxes (the discovery results); returns the annotation list.  segmentation=True: records with their masks' run-length strings,
        made without the masks; out_path: the list is also written there as the reference writes `object_discovery_with_scores.json`."""
        out = []
        for image_id, image in images:
            if str(image_id) not in raw_annotations:
                continue
            scored = self.score_image(image, raw_annotations[str(image_id)], segmentation=segmentation, masks=not segmentation)
            out.extend(self.annotations(image_id, scored))
        if out_path is not None:
            write_annotations(out, out_path)
        return out
