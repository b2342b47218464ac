"""The host form of unmore_amd.detector_input (shared by the CPU and GPU tests): every step restated in NumPy / plain Python, nothing from
the module under test.

axis_table / resize_bilinear     PIL's Image.resize((w, h), BILINEAR) on 8-bit data: the coefficient tables of one axis, in doubles, loop
                                 by loop; two passes (horizontal first) with a uint8 intermediate; a pass whose axis keeps its size is
                                 skipped.
nearest_table / resize_nearest   PIL's Image.resize(NEAREST): the source index is the truncation of a double that starts at 0.5 * a and
                                 grows by repeated addition of a = in / out.  nearest_table_mul is the (i + 0.5) * a form it is NOT.
output_shape / draw              ResizeShortestEdge.get_output_shape and the mapper's draws (augmentation_impl.py:105-223).
convert_box / transform_boxes    BoxMode.convert to XYXY_ABS, then apply_box of the resize and the flip, the clip, float32.
map_reference                    DatasetMapper.__call__ for one image on arrays (dataset_mapper.py:152-213).
normalize_pad                    GeneralizedRCNN.preprocess_image (rcnn.py:229-240) with ImageList.from_tensors' padding rule.
load_fixture                     tests/golden/det_input.npz (make_golden_det_input.py: the reference's own code on the CPU)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "det_input.npz")
XYXY_ABS, XYWH_ABS = 0, 1                      # Detectron2's BoxMode values
PRECISION_BITS = 22                            # 32 - 8 - 2: PIL's fixed point for 8-bit channels
FLIP_NONE, FLIP_H, FLIP_V = 0, 1, 2

# the ragged batch of the device tests and of the PIL comparison: (H, W) -> (new_h, new_w); see resize_cases()
WIDTHS, HEIGHTS = (1, 63, 64, 65, 130, 131), (1, 7, 48)
FULL_SCALE = (((480, 640), (240, 320)), ((375, 500), (800, 1067)), ((427, 640), (1024, 1535)))
NEAREST_PAIR = (14, 5)                         # (in, out): the first pair whose repeated-addition table differs from (i + 0.5) * a


def axis_table(inn, out):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter: (lo [out], n [out], k [out][ksize] int32)"""
    scale = float(inn) / out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    lo, n, k = np.zeros(out, np.int64), np.zeros(out, np.int64), np.zeros((out, ksize), np.int32)
    for i in range(out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), inn) - xmin
        ws, ww = [], 0.0
        for j in range(xmax):
            x = abs((j + xmin - center + 0.5) * ss)
            w = 1.0 - x if x < 1.0 else 0.0
            ws.append(w)
            ww += w
        for j in range(xmax):
            w = ws[j] / ww if ww != 0.0 else ws[j]
            k[i, j] = int(0.5 + w * (1 << PRECISION_BITS))      # bilinear weights are never negative
        lo[i], n[i] = xmin, xmax
    return lo, n, k


def _pass(a, axis, out):
    """one pass along `axis` of a uint8 array: clip((2^21 + sum_j in[lo + j] * k_j) >> 22)"""
    lo, n, k = axis_table(a.shape[axis], out)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    acc = np.full((out,) + a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    tail = (1,) * (a.ndim - 1)
    for j in range(k.shape[1]):
        idx = np.minimum(lo + j, a.shape[0] - 1)
        kj = np.where(j < n, k[:, j], 0).astype(np.int64)
        acc += a[idx] * kj.reshape((out,) + tail)
    return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def resize_bilinear(img, new_h, new_w):
    """uint8 [H,W,C] or [H,W] -> [new_h,new_w,(C)]"""
    a = np.ascontiguousarray(img)
    assert a.dtype == np.uint8
    if a.shape[1] != new_w:
        a = _pass(a, 1, new_w)
    if a.shape[0] != new_h:
        a = _pass(a, 0, new_h)
    return a.copy()


def nearest_table(inn, out):
    """the source index of every output index: truncation of 0.5 * a + a + a + ... (ImagingScaleAffine's xo += a[0])"""
    a = float(inn) / out
    t = np.zeros(out, np.int64)
    x = 0.5 * a
    for i in range(out):
        t[i] = int(x)
        x += a
    return t


def nearest_table_mul(inn, out):
    a = float(inn) / out
    return np.array([int((i + 0.5) * a) for i in range(out)], dtype=np.int64)


def resize_nearest(m, new_h, new_w):
    """[..., H, W] -> [..., new_h, new_w] (any dtype)"""
    m = np.asarray(m)
    ty, tx = nearest_table(m.shape[-2], new_h), nearest_table(m.shape[-1], new_w)
    assert ty.max(initial=0) < m.shape[-2] and tx.max(initial=0) < m.shape[-1]
    return m[..., ty, :][..., tx]


def flip_last(a, flip):
    """flip of an array whose last two axes are (y, x)"""
    return a[..., ::-1] if flip == FLIP_H else a[..., ::-1, :] if flip == FLIP_V else a


def output_shape(h, w, size, max_size):
    size = size * 1.0
    scale = size / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def draw(sizes, min_size, max_size, sample_style, flip, is_train, rs):
    """[(size, new_h, new_w, flip code)] from the RandomState `rs`, in the mapper's order"""
    out = []
    for h, w in sizes:
        size = rs.randint(min_size[0], min_size[1] + 1) if sample_style == "range" else rs.choice(min_size)
        nh, nw = (h, w) if size == 0 else output_shape(h, w, size, max_size)
        f = FLIP_NONE
        if is_train and flip != "none" and rs.uniform(0, 1) < 0.5:
            f = FLIP_H if flip == "horizontal" else FLIP_V
        out.append((int(size), nh, nw, f))
    return out


def convert_box(bbox, mode):
    """BoxMode.convert(bbox, mode, XYXY_ABS) as a float64 array.  Detectron2 takes a list / tuple through torch.tensor(box): floats become
    float32 there and x + w, y + h are float32 sums; an array keeps its own type; XYXY_ABS is returned untouched."""
    if mode == XYXY_ABS:
        return np.asarray(bbox, dtype=np.float64)
    assert mode == XYWH_ABS
    a = np.array(bbox)
    if isinstance(bbox, (list, tuple)) and a.dtype.kind == "f":
        a = a.astype(np.float32)
    a[2] += a[0]
    a[3] += a[1]
    return a.astype(np.float64)


def transform_boxes(boxes, h, w, new_h, new_w, flip):
    """float64 XYXY [N,4] -> float32 [N,4]: apply_box of the resize, then of the flip (each: the four corners through apply_coords, min and
    max), .clip(min=0), np.minimum with (new_w, new_h, new_w, new_h), Boxes' float32"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)

    def apply_box(b, coords_fn):
        c = b[:, [0, 1, 2, 1, 0, 3, 2, 3]].reshape(-1, 2).copy()
        c = coords_fn(c).reshape(-1, 4, 2)
        return np.concatenate([c.min(axis=1), c.max(axis=1)], axis=1)

    def resize(c):
        c[:, 0] = c[:, 0] * (new_w * 1.0 / w)
        c[:, 1] = c[:, 1] * (new_h * 1.0 / h)
        return c

    def hflip(c):
        c[:, 0] = new_w - c[:, 0]
        return c

    def vflip(c):
        c[:, 1] = new_h - c[:, 1]
        return c
    b = apply_box(b, resize)                                  # a NoOpTransform (size 0) keeps the shape: the factors are exactly 1.0
    if flip == FLIP_H:
        b = apply_box(b, hflip)
    elif flip == FLIP_V:
        b = apply_box(b, vflip)
    b = b.clip(min=0)
    return np.minimum(b, [new_w, new_h, new_w, new_h]).astype(np.float32)


def map_reference(image, annotations, transform, is_train=True, image_id=None, single_object_constraint=True):
    """One image through the mapper.  image: uint8 [H,W,3]; annotations: dicts with bbox, bbox_mode, iscrowd, optional score and
    `segmentation` as a decoded [H,W] array (non-zero = set); transform: (new_h, new_w, flip).  Returns image [3,h,w], and in training
    masks (bool), boxes, scores, classes, source, keep (over the non-crowd annotations, before filtering; the listed arrays are
    filtered), height, width, is_single_object."""
    H, W = image.shape[:2]
    new_h, new_w, flip = transform
    flip = int(flip)
    img = flip_last(resize_bilinear(image, new_h, new_w).transpose(2, 0, 1), flip)
    out = {"image": np.ascontiguousarray(img), "height": new_h if is_train else H, "width": new_w if is_train else W}
    if not is_train:
        return out
    src = [i for i, a in enumerate(annotations) if a.get("iscrowd", 0) == 0]
    annos = [annotations[i] for i in src]
    boxes = transform_boxes(np.stack([convert_box(a["bbox"], a["bbox_mode"]) for a in annos]) if annos else np.zeros((0, 4)),
                            H, W, new_h, new_w, flip)
    masks = np.zeros((len(annos), new_h, new_w), dtype=bool)
    for i, a in enumerate(annos):
        masks[i] = flip_last(resize_nearest(np.asarray(a["segmentation"]) != 0, new_h, new_w), flip)
    scores = [float(a["score"]) for a in annos if "score" in a]
    assert len(scores) in (0, len(annos))
    scores = np.asarray(scores, dtype=np.float32) if scores else np.ones(len(annos), dtype=np.float32)
    keep = ((boxes[:, 2] - boxes[:, 0]) > np.float32(1e-5)) & ((boxes[:, 3] - boxes[:, 1]) > np.float32(1e-5))
    keep &= masks.any(axis=(1, 2))
    out.update(masks=masks[keep], boxes=boxes[keep], scores=scores[keep], classes=np.zeros(int(keep.sum()), np.int64),
               source=np.asarray(src, dtype=np.int64)[keep], keep=keep, all_masks=masks, all_boxes=boxes, all_scores=scores,
               all_source=np.asarray(src, dtype=np.int64),
               is_single_object=bool(isinstance(image_id, str) and image_id.startswith("imagenet") and single_object_constraint))
    return out


def normalize_pad(images, mean, std, size_divisibility=32, pad_value=0.0):
    """uint8 [3,h,w] arrays -> (float32 [B,3,Hp,Wp], [(h, w)])"""
    mean, std = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(std, np.float32).reshape(3, 1, 1)
    sizes = [tuple(int(s) for s in im.shape[-2:]) for im in images]
    Hp, Wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if size_divisibility > 1:
        Hp = (Hp + size_divisibility - 1) // size_divisibility * size_divisibility
        Wp = (Wp + size_divisibility - 1) // size_divisibility * size_divisibility
    out = np.full((len(images), 3, Hp, Wp), pad_value, dtype=np.float32)
    for b, im in enumerate(images):
        out[b, :, :im.shape[1], :im.shape[2]] = (im.astype(np.float32) - mean) / std
    return out, sizes


def resize_cases():
    """The device test's ragged batch: [(H, W, new_h, new_w, flip)] over widths {1, 63, 64, 65, 130, 131} x heights {1, 7, 48}, the output
    shapes cycling through: upscale, mild downscale, extreme downscale (131 -> 10: many taps), identity in one axis, identity in both,
    outputs one below / at / above the tile edges (64 columns, 32 rows); each with and without the horizontal flip, the vertical flip
    once; then the shapes whose staged rows no longer fit a 32-row tile (400 -> 40 rows: a 16-row tile) nor a 64-column one (700 -> 4
    rows: one row of 16 columns), 3 -> 40, and 131 -> 10 with and without the flip."""
    cases, k = [], 0
    for H in HEIGHTS:
        for W in WIDTHS:
            shapes = [(H * 3 + 1, W * 2 + 3),                       # upscale
                      (max(H * 3 // 4, 1), max(W * 2 // 3, 1)),     # mild downscale
                      (max(H // 5, 1), max(W // 13, 1)),            # extreme downscale: 131 -> 10, 48 -> 9
                      (H, max(W // 2, 1)), (H * 2, W),              # identity in one axis
                      (H, W),                                       # identity in both
                      (31 + k % 3, 63 + k % 3)]                     # one below, at, above the tile edges
            for j in (k % 7, (k + 3) % 7):
                nh, nw = shapes[j]
                cases.append((H, W, nh, nw, FLIP_H if (k + j) % 2 else FLIP_NONE))
            k += 1
    cases.append((48, 130, 33, 65, FLIP_V))
    cases.append((3, 3, 40, 40, FLIP_H))
    cases.append((400, 9, 40, 9, FLIP_NONE))
    cases.append((700, 20, 4, 33, FLIP_H))
    cases.append((7, 131, 7, 10, FLIP_H))
    cases.append((7, 131, 7, 10, FLIP_NONE))
    cases.append((48, 64, 32, 64, FLIP_NONE))
    cases.append((48, 65, 33, 65, FLIP_H))
    return cases


def blob_masks(rng, H, W, N):
    """N seeded elliptic blobs, bool [N,H,W]"""
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((N, H, W), dtype=bool)
    for k in range(N):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(0.15, 0.5) * H + 0.6, rng.uniform(0.15, 0.5) * W + 0.6
        masks[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        masks[k, min(int(cy), H - 1), min(int(cx), W - 1)] = True
    return masks


def load_fixture():
    """tests/golden/det_input.npz -> dict: images (uint8 [H,W,3]), annotations (lists of dicts; `segmentation` a run-length record),
    image_ids, draws [(size, new_h, new_w, flip)], test_draws, expected / expected_test (per image dicts of arrays), cfg, batch, image_sizes"""
    z = np.load(GOLDEN)
    B = int(z["n_images"])
    fx = {"images": [], "annotations": [], "image_ids": [], "draws": [], "test_draws": [], "expected": [], "expected_test": []}
    for k in range(B):
        img = z[f"in{k}_image"]
        fx["images"].append(img)
        kind = int(z[f"in{k}_id_kind"])
        fx["image_ids"].append(f"imagenet_{k}" if kind == 1 else f"coco_{k}" if kind == 0 else k)
        chars, offs = z[f"in{k}_rle_chars"].tobytes().decode("ascii"), z[f"in{k}_rle_offsets"]
        annos = []
        for a in range(int(z[f"in{k}_bbox"].shape[0])):
            bbox = z[f"in{k}_bbox"][a]
            d = {"bbox": [float(v) for v in bbox] if int(z[f"in{k}_bbox_is_list"][a]) else bbox.copy(), "bbox_mode": int(z[f"in{k}_bbox_mode"][a]),
                 "iscrowd": int(z[f"in{k}_iscrowd"][a]),
                 "segmentation": {"size": [int(img.shape[0]), int(img.shape[1])], "counts": chars[offs[a]:offs[a + 1]]}}
            if int(z[f"in{k}_has_score"]):
                d["score"] = float(z[f"in{k}_score"][a])
            annos.append(d)
        fx["annotations"].append(annos)
        fx["draws"].append(tuple(int(v) for v in z[f"draw{k}"]))
        fx["test_draws"].append(tuple(int(v) for v in z[f"test_draw{k}"]))
        fx["expected"].append({key: z[f"out{k}_{key}"] for key in ("image", "masks", "boxes", "scores", "classes", "source", "keep")}
                              | {"height": int(z[f"out{k}_hw"][0]), "width": int(z[f"out{k}_hw"][1]),
                                 "is_single_object": bool(z[f"out{k}_single"])})
        fx["expected_test"].append({"image": z[f"test{k}_image"], "height": int(z[f"test{k}_hw"][0]), "width": int(z[f"test{k}_hw"][1])})
    fx["cfg"] = dict(min_size=tuple(int(v) for v in z["min_size"]), max_size=int(z["max_size"]), min_size_test=int(z["min_size_test"]),
                     max_size_test=int(z["max_size_test"]), seed=int(z["seed"]), pixel_mean=z["pixel_mean"], pixel_std=z["pixel_std"],
                     size_divisibility=int(z["size_divisibility"]), pil_version=str(z["pil_version"]))
    fx["batch"], fx["image_sizes"] = z["batch"], [tuple(int(v) for v in s) for s in z["image_sizes"]]
    return fx
