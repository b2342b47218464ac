"""Generate tests/golden/det_input.npz by running the REFERENCE's own dataset mapper and preprocess_image on the CPU.

Run where the reference tree and Pillow are at hand, never on the GPU box:
    python tests/golden/make_golden_det_input.py /path/to/reference

What executes verbatim from the reference: cad/data/dataset_mapper.py (`DatasetMapper.__call__`, `_transform_annotations`),
cad/data/detection_utils.py (`read_image`, `check_image_size`, `build_augmentation`'s two augmentations built as it builds them,
`transform_instance_annotations`, `annotations_to_instances`, `filter_empty_instances`), cad/data/transforms/__init__.py,
augmentation_impl.py (`ResizeShortestEdge`, `RandomFlip`) and transform.py (`ResizeTransform`: PIL's resizes), and
cad/modeling/meta_arch/rcnn.py (`GeneralizedRCNN.preprocess_image`, called on a stand-in `self` that carries pixel_mean, pixel_std and
the backbone's size_divisibility).  The images are written as PNG files and read back by the reference's `read_image`.

What cannot: Detectron2, fvcore and pycocotools are absent, so placeholder modules answer the files' imports with minimal stand-ins
written here by the published rules of those libraries:
  fvcore.transforms.transform           Transform (`_set_attributes`, `apply_box` = the four corners through `apply_coords`, min / max;
                                        `apply_segmentation` = `apply_image`, `register_type`), HFlipTransform, VFlipTransform, NoOpTransform,
                                        TransformList; the other names as empty classes
  detectron2.data.transforms.augmentation   Augmentation (`_init`, `_rand_range` = np.random.uniform, `__call__`), AugInput,
                                        AugmentationList, `_transform_to_aug`
  detectron2.structures                 BoxMode (`convert`: a list goes through torch.tensor, i.e. float32), Boxes (float32,
                                        `nonempty`), BitMasks (bool, `nonempty`), Instances (fields, `has`, `__getitem__`), ImageList
                                        (`from_tensors`: pad to the batch maximum rounded up to size_divisibility); the other names empty
  detectron2.config.configurable        the identity decorator (the mapper is constructed with explicit arguments)
  pycocotools.mask.decode               unmore_amd.rle.decode_numpy, Fortran-ordered as pycocotools returns it
  `cad`, `cad.data`, `cad.modeling...`  empty packages that only carry the reference's directories, so the files above are imported
                                        without the package __init__ files that pull in datasets, model zoo and the rest of Detectron2
`filter_empty_instances` is wrapped to record the keep mask it computes (the fixture's `keep` / `source`); it runs unchanged.

Eight images no larger than 64 x 96 with blob masks as run-length records; INPUT.MIN_SIZE_TRAIN / MAX_SIZE_TRAIN are small stand-ins
((24, 40, 56, 80, 120) / 100; test: 40 / 66) so the images stay small.  The seed is searched so that the draws reach: flip and no flip,
up- and down-scale, the max_size branch, and a down-scale of image 3, whose one-pixel mask then vanishes under the nearest resize.
Further: an image with no annotations, an iscrowd annotation, a degenerate box, an image that loses every instance, scores present and
absent, XYWH boxes as lists and XYXY boxes as lists and arrays, string and integer image ids.  Only arrays are stored."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from unmore_amd import rle  # noqa: E402
from det_input_common import blob_masks, draw  # noqa: E402

MIN_SIZE, MAX_SIZE, MIN_SIZE_TEST, MAX_SIZE_TEST = (24, 40, 56, 80, 120), 100, 40, 66
PIXEL_MEAN, PIXEL_STD, SIZE_DIVISIBILITY = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375], 32
SIZES = [(48, 64), (40, 56), (33, 47), (64, 96), (41, 35), (37, 61), (30, 50), (45, 63)]
COUNTS = [3, 0, 4, 3, 3, 2, 2, 3]


# ------------------------------------------------------------------------------------------------------------------ stand-ins
class Transform:
    def _set_attributes(self, params=None):
        for k, v in (params or {}).items():
            if k != "self" and not k.startswith("_"):
                setattr(self, k, v)

    def apply_box(self, box):
        idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
        coords = np.asarray(box).reshape(-1, 4)[:, idxs].reshape(-1, 2)
        coords = self.apply_coords(coords).reshape((-1, 4, 2))
        return np.concatenate((coords.min(axis=1), coords.max(axis=1)), axis=1)

    def apply_segmentation(self, segmentation):
        return self.apply_image(segmentation)

    @classmethod
    def register_type(cls, data_type, func=None):
        setattr(cls, "apply_" + data_type, func)


class HFlipTransform(Transform):
    def __init__(self, width):
        super().__init__()
        self._set_attributes(locals())

    def apply_image(self, img):
        return np.flip(img, axis=1) if img.ndim <= 3 else np.flip(img, axis=-2)

    def apply_coords(self, coords):
        coords[:, 0] = self.width - coords[:, 0]
        return coords


class VFlipTransform(Transform):
    def __init__(self, height):
        super().__init__()
        self._set_attributes(locals())

    def apply_image(self, img):
        return np.flip(img, axis=0) if img.ndim <= 3 else np.flip(img, axis=-3)

    def apply_coords(self, coords):
        coords[:, 1] = self.height - coords[:, 1]
        return coords


class NoOpTransform(Transform):
    def apply_image(self, img):
        return img

    def apply_coords(self, coords):
        return coords


class TransformList(Transform):
    def __init__(self, transforms):
        super().__init__()
        flat = []
        for t in transforms:
            flat.extend(t.transforms if isinstance(t, TransformList) else [t])
        self.transforms = [t for t in flat if not isinstance(t, NoOpTransform)]

    def _apply(self, x, meth):
        for t in self.transforms:
            x = getattr(t, meth)(x)
        return x

    def __getattribute__(self, name):                # as fvcore: every apply_* goes through the list, the inherited ones too
        if name.startswith("apply_"):
            return lambda x: self._apply(x, name)
        return super().__getattribute__(name)


class Augmentation:
    input_args = ("image",)

    def _init(self, params=None):
        for k, v in (params or {}).items():
            if k != "self" and not k.startswith("_"):
                setattr(self, k, v)

    def __call__(self, aug_input):
        tfm = self.get_transform(*[getattr(aug_input, a) for a in self.input_args])
        aug_input.transform(tfm)
        return tfm

    def _rand_range(self, low=1.0, high=None, size=None):
        if high is None:
            low, high = 0, low
        if size is None:
            size = []
        return np.random.uniform(low, high, size)


class AugInput:
    def __init__(self, image, *, boxes=None, sem_seg=None):
        self.image, self.boxes, self.sem_seg = image, boxes, sem_seg

    def transform(self, tfm):
        self.image = tfm.apply_image(self.image)
        if self.boxes is not None:
            self.boxes = tfm.apply_box(self.boxes)
        if self.sem_seg is not None:
            self.sem_seg = tfm.apply_segmentation(self.sem_seg)


class AugmentationList(Augmentation):
    def __init__(self, augs):
        super().__init__()
        self.augs = list(augs)

    def __call__(self, aug_input):
        return TransformList([a(aug_input) for a in self.augs])


class BoxMode:
    XYXY_ABS, XYWH_ABS = 0, 1

    @staticmethod
    def convert(box, from_mode, to_mode):
        if from_mode == to_mode:
            return box
        assert (from_mode, to_mode) == (BoxMode.XYWH_ABS, BoxMode.XYXY_ABS)
        original_type = type(box)
        single_box = isinstance(box, (list, tuple))
        if single_box:
            arr = torch.tensor(box)[None, :]
        elif isinstance(box, np.ndarray):
            arr = torch.from_numpy(np.asarray(box)).clone()
        else:
            arr = box.clone()
        arr[:, 2] += arr[:, 0]
        arr[:, 3] += arr[:, 1]
        if single_box:
            return original_type(arr.flatten().tolist())
        return arr.numpy() if isinstance(box, np.ndarray) else arr


class Boxes:
    def __init__(self, tensor):
        tensor = torch.as_tensor(tensor, dtype=torch.float32)
        self.tensor = tensor.reshape((-1, 4)) if tensor.numel() == 0 else tensor

    def nonempty(self, threshold=0.0):
        b = self.tensor
        return ((b[:, 2] - b[:, 0]) > threshold) & ((b[:, 3] - b[:, 1]) > threshold)

    def __getitem__(self, item):
        return Boxes(self.tensor[item].view(-1, 4))

    def __len__(self):
        return self.tensor.shape[0]


class BitMasks:
    def __init__(self, tensor):
        self.tensor = torch.as_tensor(tensor, dtype=torch.bool)

    def nonempty(self):
        return self.tensor.flatten(1).any(dim=1)

    def __getitem__(self, item):
        return BitMasks(self.tensor[item].view(-1, *self.tensor.shape[1:]))

    def __len__(self):
        return self.tensor.shape[0]


class Instances:
    def __init__(self, image_size, **fields):
        self._image_size, self._fields = image_size, dict(fields)

    def __setattr__(self, name, value):
        if name.startswith("_"):
            super().__setattr__(name, value)
        else:
            self._fields[name] = value

    def __getattr__(self, name):
        if name == "_fields" or name not in self._fields:
            raise AttributeError(name)
        return self._fields[name]

    def has(self, name):
        return name in self._fields

    def __len__(self):
        for v in self._fields.values():
            return len(v)
        return 0

    def __getitem__(self, item):
        return Instances(self._image_size, **{k: v[item] for k, v in self._fields.items()})


class ImageList:
    def __init__(self, tensor, image_sizes):
        self.tensor, self.image_sizes = tensor, image_sizes

    @staticmethod
    def from_tensors(tensors, size_divisibility=0, pad_value=0.0, padding_constraints=None):
        assert padding_constraints is None
        image_sizes = [(im.shape[-2], im.shape[-1]) for im in tensors]
        max_size = torch.stack([torch.as_tensor(s) for s in image_sizes]).max(0).values
        if size_divisibility > 1:
            stride = size_divisibility
            max_size = (max_size + (stride - 1)).div(stride, rounding_mode="floor") * stride
        batched = tensors[0].new_full([len(tensors), tensors[0].shape[0], int(max_size[0]), int(max_size[1])], pad_value)
        for i, img in enumerate(tensors):
            batched[i, ..., :img.shape[-2], :img.shape[-1]].copy_(img)
        return ImageList(batched.contiguous(), image_sizes)


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, m)
    return m


def _empty(name):
    return type(name, (), {})


def load_reference(ref_root):
    """(cad.data.dataset_mapper, cad.data.detection_utils, cad.data.transforms, cad.modeling.meta_arch.rcnn) of the reference"""
    tnames = ("BlendTransform", "CropTransform", "PadTransform", "GridSampleTransform", "ScaleTransform")
    fv = dict(Transform=Transform, HFlipTransform=HFlipTransform, VFlipTransform=VFlipTransform, NoOpTransform=NoOpTransform,
              TransformList=TransformList, **{n: type(n, (Transform,), {}) for n in tnames})
    fv["__all__"] = sorted(fv)
    _module("fvcore")
    _module("fvcore.transforms")
    _module("fvcore.transforms.transform", **fv)
    _module("detectron2")
    _module("detectron2.config", configurable=lambda f=None, **kw: f if f is not None else (lambda g: g))
    _module("detectron2.data")
    _module("detectron2.data.transforms")
    aug = dict(Augmentation=Augmentation, AugInput=AugInput, AugmentationList=AugmentationList, _transform_to_aug=lambda t: t)
    _module("detectron2.data.transforms.augmentation", __all__=["Augmentation", "AugInput", "AugmentationList"], **aug)
    _module("detectron2.data.catalog", MetadataCatalog=None)
    _module("detectron2.data.detection_utils", convert_image_to_rgb=None)
    _module("detectron2.structures", Boxes=Boxes, BoxMode=BoxMode, BitMasks=BitMasks, Instances=Instances, ImageList=ImageList,
            Keypoints=_empty("Keypoints"), PolygonMasks=_empty("PolygonMasks"), RotatedBoxes=_empty("RotatedBoxes"), polygons_to_bitmask=None)
    _module("detectron2.utils")
    _module("detectron2.utils.env", fixup_module_metadata=lambda *a, **k: None)
    _module("detectron2.utils.file_io", PathManager=types.SimpleNamespace(open=open))
    _module("detectron2.utils.events", get_event_storage=None)
    _module("detectron2.utils.logger", log_first_n=None)
    _module("detectron2.layers", move_device_like=lambda src, dst: src.to(dst.device))
    _module("detectron2.modeling")
    _module("detectron2.modeling.backbone", Backbone=_empty("Backbone"), build_backbone=None)
    _module("detectron2.modeling.postprocessing", detector_postprocess=None)
    _module("detectron2.modeling.proposal_generator", build_proposal_generator=None)
    _module("pycocotools")
    _module("pycocotools.mask", decode=lambda r: np.asfortranarray(rle.decode_numpy(rle.as_record(r))))
    for pkg, sub in (("cad", "cad"), ("cad.data", "cad/data"), ("cad.modeling", "cad/modeling"), ("cad.modeling.meta_arch", "cad/modeling/meta_arch")):
        _module(pkg).__path__ = [os.path.join(ref_root, sub)]
    _module("cad.modeling.roi_heads", build_roi_heads=None)
    registry = types.SimpleNamespace(register=lambda: (lambda cls: cls))
    _module("cad.modeling.meta_arch.build", META_ARCH_REGISTRY=registry)
    T = importlib.import_module("cad.data.transforms")
    utils = importlib.import_module("cad.data.detection_utils")
    mapper = importlib.import_module("cad.data.dataset_mapper")
    rcnn = importlib.import_module("cad.modeling.meta_arch.rcnn")
    for m in (T, utils, mapper, rcnn):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_root)), m.__file__
    return mapper, utils, T, rcnn


# ------------------------------------------------------------------------------------------------------------------ the batch
def build_inputs(seed, draws):
    """images (uint8 [H,W,3]), per image the annotation dicts (masks as run-length records) and the image ids"""
    rng = np.random.RandomState(2000 + seed)
    images, annos, ids = [], [], []
    for k, ((H, W), n) in enumerate(zip(SIZES, COUNTS)):
        # 8 x 8 blocks of random colour with a ramp across a quarter of the frame: edges and slopes for the resize, and a file that compresses
        img = np.kron(rng.randint(0, 256, (-(-H // 8), -(-W // 8), 3)), np.ones((8, 8, 1), dtype=np.int64))[:H, :W].astype(np.uint8)
        img[:H // 2, :W // 2, k % 3] = (np.arange(W // 2) * 255 // max(W // 2 - 1, 1)).astype(np.uint8)[None, :]
        masks = blob_masks(rng, H, W, n)
        if k == 3:                                   # one pixel that the nearest tables of this image's draw do not sample
            from det_input_common import nearest_table
            _, nh, nw, _ = draws[3]
            ty, tx = set(nearest_table(H, nh).tolist()), set(nearest_table(W, nw).tolist())
            y = next(v for v in range(H // 2, H) if v not in ty)
            x = next(v for v in range(W // 2, W) if v not in tx)
            masks[1] = False
            masks[1, y, x] = True
        if k == 5:                                   # every instance goes: an empty mask, and a box without width
            masks[0] = False
        objs = []
        for j in range(n):
            ys, xs = np.nonzero(masks[j])
            if ys.size:
                x0, y0, x1, y1 = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
            else:
                x0, y0, x1, y1 = 3, 4, 9, 11
            jit = rng.uniform(0, 0.9, 4)
            if (k + j) % 2 == 0:
                bbox, mode = [float(x0 + jit[0]), float(y0 + jit[1]), float(x1 - x0 + jit[2]), float(y1 - y0 + jit[3])], BoxMode.XYWH_ABS
            else:
                bbox, mode = [float(x0 + jit[0]), float(y0 + jit[1]), float(x1 + jit[2]), float(y1 + jit[3])], BoxMode.XYXY_ABS
                if k == 4:
                    bbox = np.array(bbox)
            obj = {"bbox": bbox, "bbox_mode": mode, "iscrowd": 0, "segmentation": rle.encode_numpy(masks[j].astype(np.uint8)),
                   "category_id": 0}
            if k in (2, 6):
                obj["score"] = float(np.float32(rng.uniform(0.05, 1.0)))
            objs.append(obj)
        if k == 2:
            objs[1]["iscrowd"] = 1
        if k == 4:                                   # a degenerate box: no width
            b = objs[2]["bbox"]
            objs[2]["bbox"], objs[2]["bbox_mode"] = np.array([b[0], b[1], b[0], b[3] + 2.0]), BoxMode.XYXY_ABS
        if k == 5:
            b = objs[1]["bbox"]
            objs[1]["bbox"], objs[1]["bbox_mode"] = [float(b[0]), float(b[1]), 0.0, 5.5], BoxMode.XYWH_ABS
        images.append(img)
        annos.append(objs)
        ids.append(f"imagenet_{k}" if k in (1, 2, 6) else k if k == 5 else f"coco_{k}")
    return images, annos, ids


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import PIL
    from PIL import Image
    if not hasattr(Image, "LINEAR"):                 # transform.py names it in a default argument; recent Pillow calls it BILINEAR only
        Image.LINEAR = Image.BILINEAR
    mapper_mod, utils, T, rcnn = load_reference(sys.argv[1])
    kept = []
    orig_filter = utils.filter_empty_instances

    def recording_filter(instances, **kw):
        out, m = orig_filter(instances, return_mask=True, **kw)
        kept.append(m.numpy().copy())
        return out
    utils.filter_empty_instances = recording_filter

    for seed in range(10000):
        draws = draw(SIZES, MIN_SIZE, MAX_SIZE, "choice", "horizontal", True, np.random.RandomState(seed))
        flips = [d[3] for d in draws]
        ups = [d[1] > h for d, (h, w) in zip(draws, SIZES)]
        capped = [d[0] * 1.0 / min(h, w) * max(h, w) > MAX_SIZE for d, (h, w) in zip(draws, SIZES)]
        if not (0 < sum(flips) < len(flips) and any(ups) and not all(ups) and any(capped) and draws[3][0] < 64 and flips[3] and not flips[4]):
            continue
        images, annos, ids = build_inputs(seed, draws)
        arrays = {"seed": np.int64(seed), "n_images": np.int64(len(SIZES)), "min_size": np.array(MIN_SIZE, dtype=np.int64),
                  "max_size": np.int64(MAX_SIZE), "min_size_test": np.int64(MIN_SIZE_TEST), "max_size_test": np.int64(MAX_SIZE_TEST),
                  "pixel_mean": np.array(PIXEL_MEAN), "pixel_std": np.array(PIXEL_STD), "size_divisibility": np.int64(SIZE_DIVISIBILITY),
                  "pil_version": np.array(PIL.__version__)}
        with tempfile.TemporaryDirectory() as tmp:
            dicts = []
            for k, img in enumerate(images):
                path = os.path.join(tmp, f"{k}.png")
                Image.fromarray(img).save(path)
                dicts.append({"file_name": path, "image_id": ids[k], "height": img.shape[0], "width": img.shape[1], "annotations": annos[k]})
            # build_augmentation (detection_utils.py:625-649) with the stand-in sizes, the recipe's sampling and flip
            train_augs = [T.ResizeShortestEdge(MIN_SIZE, MAX_SIZE, "choice"), T.RandomFlip(horizontal=True, vertical=False)]
            test_augs = [T.ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST, "choice")]
            common = dict(image_format="RGB", use_instance_mask=True, instance_mask_format="bitmask", recompute_boxes=False,
                          imagenet_single_object_constraint=True)
            train = mapper_mod.DatasetMapper(True, augmentations=train_augs, **common)
            test = mapper_mod.DatasetMapper(False, augmentations=test_augs, **common)
            np.random.seed(seed)
            outs = [train(d) for d in dicts]
            test_draws = draw(SIZES, (MIN_SIZE_TEST, MIN_SIZE_TEST), MAX_SIZE_TEST, "choice", "none", False, np.random.RandomState(seed + 1))
            np.random.seed(seed + 1)
            touts = [test(d) for d in dicts]
            for k, img in enumerate(images):
                assert np.array_equal(utils.read_image(dicts[k]["file_name"], "RGB"), img)
        assert len(kept) == len(SIZES)
        for k, (img, objs, o, t) in enumerate(zip(images, annos, outs, touts)):
            inst = o["instances"]
            assert tuple(o["image"].shape[1:]) == draws[k][1:3] and tuple(t["image"].shape[1:]) == test_draws[k][1:3], (k, o["image"].shape)
            noncrowd = [j for j, a in enumerate(objs) if a["iscrowd"] == 0]
            chars = "".join(a["segmentation"]["counts"] for a in objs)
            arrays[f"in{k}_image"] = img
            arrays[f"in{k}_id_kind"] = np.int64(1 if isinstance(ids[k], str) and ids[k].startswith("imagenet") else 0 if isinstance(ids[k], str) else 2)
            arrays[f"in{k}_bbox"] = np.array([np.asarray(a["bbox"], dtype=np.float64) for a in objs]).reshape(-1, 4)
            arrays[f"in{k}_bbox_is_list"] = np.array([isinstance(a["bbox"], list) for a in objs], dtype=np.int64)
            arrays[f"in{k}_bbox_mode"] = np.array([a["bbox_mode"] for a in objs], dtype=np.int64)
            arrays[f"in{k}_iscrowd"] = np.array([a["iscrowd"] for a in objs], dtype=np.int64)
            arrays[f"in{k}_has_score"] = np.int64(bool(objs) and "score" in objs[0])
            arrays[f"in{k}_score"] = np.array([a.get("score", 1.0) for a in objs], dtype=np.float64)
            arrays[f"in{k}_rle_chars"] = np.frombuffer(chars.encode("ascii"), dtype=np.uint8)
            arrays[f"in{k}_rle_offsets"] = np.concatenate([[0], np.cumsum([len(a["segmentation"]["counts"]) for a in objs])]).astype(np.int64)
            arrays[f"draw{k}"] = np.array(draws[k], dtype=np.int64)
            arrays[f"test_draw{k}"] = np.array(test_draws[k], dtype=np.int64)
            arrays[f"out{k}_image"] = o["image"].numpy()
            n = len(inst)
            arrays[f"out{k}_masks"] = inst.gt_masks.tensor.numpy() if inst.has("gt_masks") else np.zeros((0,) + draws[k][1:3], dtype=bool)
            arrays[f"out{k}_boxes"] = inst.gt_boxes.tensor.numpy()
            arrays[f"out{k}_scores"] = inst.gt_scores.numpy()
            arrays[f"out{k}_classes"] = inst.gt_classes.numpy()
            arrays[f"out{k}_keep"] = kept[k]
            arrays[f"out{k}_source"] = np.asarray(noncrowd, dtype=np.int64)[kept[k]]
            assert arrays[f"out{k}_source"].size == n
            arrays[f"out{k}_hw"] = np.array([o["height"], o["width"]], dtype=np.int64)
            arrays[f"out{k}_single"] = np.int64(o["is_single_object"])
            arrays[f"test{k}_image"] = t["image"].numpy()
            arrays[f"test{k}_hw"] = np.array([t["height"], t["width"]], dtype=np.int64)
            assert "instances" not in t and "annotations" not in t
        # the branches, asserted on the reference's own outputs
        assert len(outs[1]["instances"]) == 0 and len(outs[5]["instances"]) == 0
        assert kept[3].tolist() == [True, False, True] and kept[4].tolist() == [True, True, False] and len(kept[2]) == 3, [m.tolist() for m in kept]
        assert outs[1]["is_single_object"] and not outs[0]["is_single_object"] and not outs[5]["is_single_object"]
        # preprocess_image on a stand-in self
        me = types.SimpleNamespace(pixel_mean=torch.tensor(PIXEL_MEAN).view(-1, 1, 1), pixel_std=torch.tensor(PIXEL_STD).view(-1, 1, 1),
                                   backbone=types.SimpleNamespace(size_divisibility=SIZE_DIVISIBILITY, padding_constraints=None))
        me._move_to_current_device = lambda x: rcnn.GeneralizedRCNN._move_to_current_device(me, x)
        il = rcnn.GeneralizedRCNN.preprocess_image(me, outs)
        arrays["batch"] = il.tensor.numpy()
        arrays["image_sizes"] = np.array(il.image_sizes, dtype=np.int64)
        path = os.path.join(HERE, "det_input.npz")
        np.savez_compressed(path, **arrays)
        print(f"seed {seed}: wrote {path} ({os.path.getsize(path)} bytes); draws {draws}; kept {[m.tolist() for m in kept]}; "
              f"batch {tuple(il.tensor.shape)}")
        return
    sys.exit("no seed reaches every branch")


if __name__ == "__main__":
    main()
