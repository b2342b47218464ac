"""The VoteCut annotation file (COCO layout: `images`, `annotations` with `image_id`, `weight` and a run-length `segmentation`) as
the source of the existence classifier's and ObjectnessNet's training masks -- what the reference makes offline with
utils/preprocess_votecut.py (top-1 annotation, largest 4-connected component, written as mask * 255) and utils/vis_votecut.py (all of an
image's annotations in one PNG, of which datasets.py:297-298 reads `> 0`: their union).  Here the strings go to the device and the
masks are made there (rle.largest_component, rle.decode): annotations -> masks -> synthesize_*_items -> train step with nothing
image-sized crossing the host."""
import json

from . import rle


class VoteCutAnnotations:
    def __init__(self, path_or_dict):
        if isinstance(path_or_dict, dict):
            d = path_or_dict
        else:
            with open(path_or_dict) as f:
                d = json.load(f)
        self._file_name = {im["id"]: im["file_name"] for im in d["images"]}                 # preprocess_votecut.py:57-60
        self._anns = {}
        for ann in d["annotations"]:                                                         # :63-69, file order inside an image
            self._anns.setdefault(ann["image_id"], []).append(ann)
        self.image_ids = sorted(self._anns)                                                  # :71: the ids that have an annotation

    def __len__(self):
        return len(self.image_ids)

    def file_name(self, image_id):
        return self._file_name[image_id]

    def top1(self, image_id):
        """the first annotation of maximal weight in file order (np.argmax of the weights, :74-79)"""
        anns = self._anns[image_id]
        best = anns[0]
        for ann in anns[1:]:
            if ann["weight"] > best["weight"]:
                best = ann
        return best

    def records(self, image_id):
        """the run-length records of all of the image's annotations, in file order"""
        return [ann["segmentation"] for ann in self._anns[image_id]]

    def masks(self, image_ids, device="cuda"):
        """(top1_masks, full_masks) for the images: two lists of [h, w] u8 device tensors holding 0 / 255, the lists
        synthesize_training_items(images, top1_masks, ...) and synthesize_classifier_items(images, top1_masks, full_masks, ...) take.
        top1_masks: the largest 4-connected component of the top-1 annotation; full_masks: the union of the image's annotations.  Two
        umr_rle_decode calls; each reads its status words back once.  A mask stored transposed relative to its image is rotated by
        the caller (torch.rot90(mask, -1)), as those functions' docstrings say."""
        image_ids = list(image_ids)
        top1, _ = rle.largest_component([self.top1(i)["segmentation"] for i in image_ids], device=device)
        records, groups = [], []
        for i in image_ids:
            recs = self.records(i)
            size = recs[0]["size"] if isinstance(recs[0], dict) and "size" in recs[0] else None
            if size is None:
                raise ValueError(f"VoteCutAnnotations.masks: image {i}: only run-length segmentations are decoded")
            records += recs
            groups.append((len(recs), (size[0], size[1])))
        full = rle.decode(records, groups=groups, device=device)
        return top1, full
