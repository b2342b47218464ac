"""The stage-3 detector's input path on the device: the dataset mapper's resize and flip of a decoded image and its instance masks, and the
model's normalise + pad + batch.  Bit-exact: PIL's 8-bit resize is fixed-point integer arithmetic, its nearest resize a table lookup, the
normalisation one float32 subtract and one float32 divide.  The planned chain: rle.decode -> map_batch -> copy_and_paste ->
preprocess_image -> backbone -> rpn -> ...

What is reproduced (the reference's recipe: INPUT.MIN_SIZE_TRAIN (240 ... 1024), MAX_SIZE_TRAIN 1333, MASK_FORMAT "bitmask"):
  DatasetMapper.__call__                 cad/data/dataset_mapper.py:152-213 (and _transform_annotations, :123-150)
  build_augmentation                     cad/data/detection_utils.py:625-649: ResizeShortestEdge, then RandomFlip in training
  RandomFlip, ResizeShortestEdge         cad/data/transforms/augmentation_impl.py:105-134, 157-223
  ResizeTransform                        cad/data/transforms/transform.py:94-163 (PIL Image.resize on uint8; apply_coords)
  transform_instance_annotations         cad/data/detection_utils.py:262-323
  annotations_to_instances               cad/data/detection_utils.py:374-450
  filter_empty_instances                 cad/data/detection_utils.py:482-515
  GeneralizedRCNN.preprocess_image       cad/modeling/meta_arch/rcnn.py:229-240 (ImageList.from_tensors' padding rule)

Draws (`draw_transforms`, host): per image, from the one numpy stream and in the reference's order, size = np_random.choice(min_size)
("choice") or randint(lo, hi + 1) ("range"), then in training, if flipping is on, np_random.uniform(0, 1) < 0.5.  size == 0: no resize.
The output shape is ResizeShortestEdge.get_output_shape in Python doubles, the max_size rescale and int(x + 0.5) included.

Image = PIL Image.resize((new_w, new_h), BILINEAR) on uint8 RGB: two separable passes, horizontal first, the intermediate rounded and
clipped to uint8 (the passes cannot be merged); a pass whose axis keeps its size is skipped.  Per axis with sizes in, out: scale = in /
out, fs = max(scale, 1), support = fs; for output i: center = (i + 0.5) * scale, lo = max(int(center - support + 0.5), 0), n =
min(int(center + support + 0.5), in) - lo, w_j = max(0, 1 - |(j + lo - center + 0.5) * (1 / fs)|) (PIL multiplies by the reciprocal),
summed sequentially in double, each divided by the sum, k_j = int(0.5 + w_j * 2^22); byte = clip((2^21 + sum_j in[lo + j] * k_j) >> 22,
0, 255).  The tables are built here in float64 and uploaded; the device side is integer only.

Mask = PIL Image.resize(NEAREST): out[y, x] = in[ty[y], tx[x]], the source index the truncation of a double that starts at 0.5 * a and
grows by REPEATED ADDITION of a = in / out (not (i + 0.5) * a: the two differ for some sizes, 14 -> 5 is the smallest).

Flip after the resize (HFlipTransform: out[..., x] = resized[..., new_w - 1 - x]; VFlipTransform likewise in y).

Boxes (host, float64, a few dozen values per image; they travel up in the call's table buffer): BoxMode.convert to XYXY_ABS -- Detectron2
takes a list or tuple through torch.tensor(box), so its floats are rounded to float32 and x + w, y + h are float32 sums; an array keeps
its type; an XYXY_ABS box is returned untouched -- then apply_box of the resize (x * (new_w * 1.0 / w), y * (new_h * 1.0 / h)) and of the
flip (new_w - x) on the four corners with min / max, .clip(min=0), np.minimum(box, [new_w, new_h, new_w, new_h]), float32.

Instances: annotations with iscrowd != 0 are dropped first; gt_classes are zero; gt_scores come from "score" if present, else ones (the
reference breaks if only some annotations carry a score: ValueError here); filter_empty_instances keeps an instance iff its float32 box
has width and height > 1e-5 and its resized mask has a set pixel.  height / width are the new shape in training and the original
shape at test time; is_single_object follows dataset_mapper.py:202-211.

preprocess_image: (float32(u8) - mean[c]) / std[c] per image into [B, 3, Hp, Wp] float32, Hp / Wp the batch maxima rounded up to
size_divisibility when it is > 1, images at the top left, pad_value elsewhere.

Three kernels (csrc/det_input.hip), each one launch for the whole ragged batch.  No CPU fallback: tests/det_input_common.py is the host
form.  Out of scope: JPEG / PNG decoding, RandomCrop, the float-image F.interpolate branch of ResizeTransform.apply_image, polygons,
keypoints, sem_seg and precomputed proposals (ValueError)."""
import ctypes

import numpy as np

LDS_PIX, MAX_TW, NN_BAND = 10880, 64, 4096      # csrc/det_input.hip: DI_LDS_PIX, DI_MAX_TW, NN_BAND
TILE_ROWS = (32, 16, 8, 4, 2, 1)
PRECISION_BITS = 22
FLIP_NONE, FLIP_H, FLIP_V = 0, 1, 2
XYXY_ABS, XYWH_ABS = 0, 1                       # Detectron2's BoxMode values
BOX_THRESHOLD = np.float32(1e-5)
MIN_SIZE_TRAIN = (240, 320, 480, 640, 672, 704, 736, 768, 800, 1024)     # the recipe's INPUT.MIN_SIZE_TRAIN (MAX_SIZE_TRAIN: 1333)
_BL, _NN, _NP = 16, 13, 4                       # descriptor widths (int64 fields per image)
DIRECT_BYTES = 1 << 18                          # a host input of this size or more goes up in a copy of its own (see _sources)


# ---------------------------------------------------------------------------------------------------------------- draws and tables (host)
def output_shape(h, w, size, max_size):
    """ResizeShortestEdge.get_output_shape (augmentation_impl.py:203-223)"""
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


def draw_transforms(sizes, *, min_size, max_size=1333, sample_style="choice", flip="horizontal", is_train=True, np_random=np.random):
    """The mapper's draws for a batch.  sizes[i]: (H, W) of image i.  Returns (new_h, new_w, flip) per image, flip = 0 (none), 1
    (horizontal) or 2 (vertical).  min_size: an int or a sequence (two values for "range"); flip: "horizontal", "vertical" or "none";
    at test time (is_train=False) there is no flip draw.  np_random: `numpy.random` or a RandomState."""
    if sample_style not in ("choice", "range"):
        raise ValueError(f"draw_transforms: sample_style must be 'choice' or 'range', got {sample_style!r}")
    if flip not in ("horizontal", "vertical", "none"):
        raise ValueError(f"draw_transforms: flip must be 'horizontal', 'vertical' or 'none', got {flip!r}")
    if isinstance(min_size, (int, np.integer)):
        min_size = (int(min_size), int(min_size))
    min_size = tuple(int(s) for s in min_size)
    if sample_style == "range" and len(min_size) != 2:
        raise ValueError(f"draw_transforms: min_size must be two values with the 'range' sample style, got {min_size}")
    if not min_size or min(min_size) < 0:
        raise ValueError(f"draw_transforms: min_size must hold non-negative sizes, got {min_size}")
    out = []
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"draw_transforms: sizes[{i}] = {(h, w)} is not positive")
        size = int(np_random.randint(min_size[0], min_size[1] + 1)) if sample_style == "range" else int(np_random.choice(min_size))
        nh, nw = (h, w) if size == 0 else output_shape(h, w, size, max_size)
        f = FLIP_NONE
        if is_train and flip != "none" and np_random.uniform(0, 1) < 0.5:
            f = FLIP_H if flip == "horizontal" else FLIP_V
        out.append((nh, nw, f))
    return out


def bilinear_table(inn, out):
    """PIL's coefficients of one axis (precompute_coeffs + normalize_coeffs_8bpc, bilinear filter): (lo int32 [out], n int32 [out], k
    int32 [out][ksize]); an axis that keeps its size gets the table that returns the byte itself (PIL skips that pass)"""
    if inn == out:
        return np.arange(out, dtype=np.int32), np.ones(out, dtype=np.int32), np.full((out, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = float(inn) / out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)            # astype truncates toward zero, as C's (int) does
    n = np.minimum((center + support + 0.5).astype(np.int64), inn) - lo
    j = np.arange(ksize, dtype=np.int64)[None, :]
    x = np.abs(((j + lo[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where((x < 1.0) & (j < n[:, None]), 1.0 - x, 0.0)
    ww = np.zeros(out, dtype=np.float64)
    for q in range(ksize):                                                   # the sum in PIL's order; the zeros past n change nothing
        ww = ww + w[:, q]
    w = w / np.where(ww != 0.0, ww, 1.0)[:, None]
    k = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)
    k[j >= n[:, None]] = 0
    return lo.astype(np.int32), n.astype(np.int32), k


def nearest_table(inn, out):
    """PIL's nearest source indices of one axis: truncation of 0.5 * a, + a, + a, ... in doubles (np.add.accumulate adds in order)"""
    a = float(inn) / out
    steps = np.full(out, a, dtype=np.float64)
    steps[0] = 0.5 * a
    return np.minimum(np.add.accumulate(steps).astype(np.int64), inn - 1).astype(np.int32)


def tile_shape(vlo, vn, new_h):
    """(TH, TW) of the bilinear kernel's output tile: the largest row count whose staged input rows fit the LDS budget at 64 columns,
    else one row of fewer columns"""
    vlo, vn = vlo.astype(np.int64), vn.astype(np.int64)
    span = 0
    for th in TILE_ROWS:
        y0 = np.arange(0, new_h, th)
        y1 = np.minimum(y0 + th, new_h) - 1
        span = int((vlo[y1] + vn[y1] - vlo[y0]).max())
        if span * MAX_TW <= LDS_PIX:
            return th, MAX_TW
    tw = MAX_TW // 2
    while tw >= 1:
        if span * tw <= LDS_PIX:
            return 1, tw
        tw //= 2
    raise ValueError(f"one output row reads {span} input rows; at most {LDS_PIX} fit")


def convert_box(bbox, mode, what="bbox"):
    """BoxMode.convert(bbox, mode, XYXY_ABS) as four doubles (see the module docstring for the float32 step of a list)"""
    mode = int(mode)
    if mode not in (XYXY_ABS, XYWH_ABS):
        raise ValueError(f"{what}: bbox_mode must be XYXY_ABS (0) or XYWH_ABS (1), got {mode}")
    a = np.array(bbox)
    if a.shape != (4,) or a.dtype.kind not in "fiu":
        raise ValueError(f"{what}: bbox must be four numbers, got {bbox!r}")
    if mode == XYXY_ABS:
        return a.astype(np.float64)
    if isinstance(bbox, (list, tuple)) and a.dtype.kind == "f":
        a = a.astype(np.float32)
    a[2] += a[0]
    a[3] += a[1]
    return a.astype(np.float64)


def transform_boxes(boxes, h, w, new_h, new_w, flip):
    """float64 XYXY [N,4] through the resize and the flip -> float32 [N,4] (TransformList.apply_box, the clip, Boxes' float32)"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    sx, sy = new_w * 1.0 / w, new_h * 1.0 / h
    xs, ys = b[:, 0::2] * sx, b[:, 1::2] * sy
    x0, x1, y0, y1 = xs.min(1), xs.max(1), ys.min(1), ys.max(1)
    if flip == FLIP_H:
        x0, x1 = np.minimum(new_w - x0, new_w - x1), np.maximum(new_w - x0, new_w - x1)
    elif flip == FLIP_V:
        y0, y1 = np.minimum(new_h - y0, new_h - y1), np.maximum(new_h - y0, new_h - y1)
    b = np.stack([x0, y0, x1, y1], 1).clip(min=0)
    return np.minimum(b, [new_w, new_h, new_w, new_h]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- argument checks
def _check_transforms(transforms, n, what):
    if len(transforms) != n:
        raise ValueError(f"{what}: {len(transforms)} transforms for {n} images")
    out = []
    for i, t in enumerate(transforms):
        try:
            nh, nw, f = t
            nh, nw, f = int(nh), int(nw), int(f)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: transforms[{i}] must be (new_h, new_w, flip)") from None
        if nh < 1 or nw < 1 or nh * nw >= 1 << 30:
            raise ValueError(f"{what}: transforms[{i}]: the shape {(nh, nw)} must be positive with fewer than 2^30 pixels")
        if f not in (FLIP_NONE, FLIP_H, FLIP_V):
            raise ValueError(f"{what}: transforms[{i}]: flip must be 0 (none), 1 (horizontal) or 2 (vertical), got {f}")
        out.append((nh, nw, f))
    return out


def _check_image(img, i, what):
    import torch
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        got = f"{img.dtype} {list(img.shape)}" if isinstance(img, torch.Tensor) else type(img).__name__
        raise ValueError(f"{what}: images[{i}] must be a uint8 [H, W, 3] tensor (PIL's layout), got {got}")
    H, W = int(img.shape[0]), int(img.shape[1])
    if H < 1 or W < 1 or H * W >= 1 << 30:
        raise ValueError(f"{what}: images[{i}]: the size {(H, W)} must be positive with fewer than 2^30 pixels")
    return H, W


def _check_masks(m, i, what):
    import torch
    if not isinstance(m, torch.Tensor) or m.dtype not in (torch.bool, torch.uint8) or m.dim() != 3:
        got = f"{m.dtype} {list(m.shape)}" if isinstance(m, torch.Tensor) else type(m).__name__
        raise ValueError(f"{what}: masks[{i}] must be a bool or uint8 [N, H, W] tensor, got {got}")
    N, H, W = (int(s) for s in m.shape)
    if H < 1 or W < 1 or H * W >= 1 << 30:
        raise ValueError(f"{what}: masks[{i}]: the size {(H, W)} must be positive with fewer than 2^30 pixels")
    return N, H, W


def _device(tensors, device, what):
    """the one GPU of a call: that of its device tensors, else `device`, else the current one"""
    import torch
    devs = {t.device for t in tensors if t.device.type != "cpu"}
    if any(d.type != "cuda" for d in devs) or not torch.cuda.is_available():
        raise RuntimeError(f"unmore_amd.detector_input.{what} runs on the MI355X only (no CPU fallback); tests/det_input_common.py restates "
                           "it on the host")
    if device is not None:
        d = torch.device(device)
        if d.type != "cuda":
            raise ValueError(f"{what}: device must be a GPU, got {d}")
        devs.add(d if d.index is not None else torch.device("cuda", torch.cuda.current_device()))
    if len(devs) > 1:
        raise ValueError(f"{what}: every device tensor must be on the same device, got {sorted(str(d) for d in devs)}")
    return devs.pop() if devs else torch.device("cuda", torch.cuda.current_device())


# ---------------------------------------------------------------------------------------------------------------- one call's buffers
class _Pack:
    """The call's table buffer, one host-to-device copy: arrays laid out 16-byte aligned in one buffer.  The device buffer exists before the copy, so
    descriptors can hold addresses inside it."""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        off = self.size
        self.parts.append((off, a))
        self.size = (off + a.nbytes + 15) & ~15
        return off

    def upload(self, dev, fill):
        """allocate, let `fill(base address)` complete the descriptors, copy"""
        import torch
        buf = torch.empty(max(self.size, 16), dtype=torch.uint8, device=dev)
        fill(buf.data_ptr())
        host = np.empty(max(self.size, 16), dtype=np.uint8)                           # the alignment gaps are never read
        for off, a in self.parts:
            host[off:off + a.nbytes] = a.view(np.uint8)
        buf.copy_(torch.from_numpy(host))
        return buf


class _Tables:
    """the int32 tables of a call, one copy per (in, out) pair"""

    def __init__(self):
        self.parts, self.size, self.bl, self.nn = [], 0, {}, {}

    def _add(self, a):
        off = self.size
        self.parts.append(np.ascontiguousarray(a, dtype=np.int32).reshape(-1))
        self.size += self.parts[-1].size
        return off

    def bilinear(self, inn, out):
        """(offset of the (lo, n) pairs, offset of the weights, ksize, lo, n)"""
        if (inn, out) not in self.bl:
            lo, n, k = bilinear_table(inn, out)
            self.bl[inn, out] = (self._add(np.stack([lo, n], 1)), self._add(k), k.shape[1], lo, n)
        return self.bl[inn, out]

    def nearest(self, inn, out):
        if (inn, out) not in self.nn:
            self.nn[inn, out] = self._add(nearest_table(inn, out))
        return self.nn[inn, out]

    def array(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(4, dtype=np.int32)


def _plan_images(tabs, sizes, transforms, what):
    """bilinear descriptors without addresses: (int64 [B][16], total tiles, output byte offsets, output bytes)"""
    desc = np.zeros((len(sizes), _BL), dtype=np.int64)
    tiles = off = 0
    offs = []
    for i, ((H, W), (nh, nw, f)) in enumerate(zip(sizes, transforms)):
        hb, hk, hks, _, _ = tabs.bilinear(W, nw)
        vb, vk, vks, vlo, vn = tabs.bilinear(H, nh)
        try:
            th, tw = tile_shape(vlo, vn, nh)
        except ValueError as e:
            raise ValueError(f"{what}: images[{i}] ({H} x {W} -> {nh} x {nw}): {e}") from None
        desc[i, 2:] = (H, W, nh, nw, f, hb, hk, hks, vb, vk, vks, th, tw, tiles)
        tiles += -(-nh // th) * -(-nw // tw)
        offs.append(off)
        off += (3 * nh * nw + 15) & ~15
    if tiles >= 1 << 31:
        raise ValueError(f"{what}: {tiles} output tiles in one call; split the batch")
    return desc, tiles, offs, off


def _plan_masks(tabs, shapes, transforms, what):
    """nearest descriptors without addresses and strides.  shapes[i]: (N, H, W).  (int64 [B][13], total workgroups, output byte offsets,
    output bytes, first flag per image, flag count)"""
    desc = np.zeros((len(shapes), _NN), dtype=np.int64)
    blocks = off = flags = 0
    offs, flag0 = [], []
    for i, ((N, H, W), (nh, nw, f)) in enumerate(zip(shapes, transforms)):
        rows = -(-(-(-NN_BAND // nw)) // 4) * 4                                    # csrc/det_input.hip: rows per workgroup, a multiple of 4
        desc[i, 2:12] = (N, H, W, nh, nw, f, tabs.nearest(W, nw), tabs.nearest(H, nh), flags, blocks)
        blocks += N * -(-nh // rows)
        offs.append(off)
        flag0.append(flags)
        off += (N * nh * nw + 15) & ~15
        flags += N
    if blocks >= 1 << 31:
        raise ValueError(f"{what}: {blocks} workgroups in one call; split the batch")
    return desc, blocks, offs, off, flag0, flags


def _sources(pack, tensors, dev):
    """Where each input tensor will be on the device.  Device tensors are read in place (('ptr', address)).  Small host tensors join the
    call's one upload (('pack', offset)); a host tensor of DIRECT_BYTES or more goes up in a copy of its own, asynchronous from pinned
    memory: packing 113 MB of images and masks into one buffer first cost 80 ms of host copies per batch of 16, the direct copies
    a few.  Returns the list and the tensors to keep alive until the launches are enqueued."""
    import torch
    where, hold = [], []
    for t in tensors:
        t = t.contiguous()
        t = t.view(torch.uint8) if t.dtype == torch.bool else t
        if t.device.type == "cpu" and t.numel() >= DIRECT_BYTES:
            t = t.to(dev, non_blocking=True)
        hold.append(t)
        if t.device.type == "cpu":
            where.append(("pack", pack.add(t.numpy())) if t.numel() else ("ptr", 0))
        else:
            where.append(("ptr", t.data_ptr() if t.numel() else 0))
    return where, hold


def _span(segs, H, W):
    """decoded masks that lie equally spaced in one storage (the slices of an [N, H, W] tensor, rle.decode's views): that storage as one
    uint8 [N, H, W] strided view, else None"""
    import torch
    u = [t.view(torch.uint8) if t.dtype == torch.bool else t for t in segs]
    if any(not t.is_contiguous() or t.device != u[0].device for t in u):
        return None
    p = [t.data_ptr() for t in u]
    stride = p[1] - p[0] if len(p) > 1 else H * W
    if stride < H * W or any(p[j + 1] - p[j] != stride for j in range(len(p) - 1)):
        return None
    if any(t.untyped_storage().data_ptr() != u[0].untyped_storage().data_ptr() for t in u):
        return None
    return torch.as_strided(u[0], (len(u), H, W), (stride, W, 1))


def _addr(where, base):
    kind, v = where
    return base + v if kind == "pack" else v


def _launch_bilinear(buf, o_desc, B, o_tab, tab_len, tiles):
    from . import _lib as L
    from .ops import _stream
    vp = ctypes.c_void_p
    L.check(L.lib().umr_det_resize_bilinear(vp(buf.data_ptr() + o_desc), B, vp(buf.data_ptr() + o_tab), tab_len, tiles, _stream()),
            "umr_det_resize_bilinear")


def _launch_nearest(buf, o_desc, B, o_tab, tab_len, blocks, flags):
    from . import _lib as L
    from .ops import _p, _stream
    vp = ctypes.c_void_p
    L.check(L.lib().umr_det_resize_nearest(vp(buf.data_ptr() + o_desc), B, vp(buf.data_ptr() + o_tab), tab_len, blocks, _p(flags),
                                           flags.numel(), _stream()), "umr_det_resize_nearest")


def _timed(fn, name, phase_ms):
    """fn() -- between device events when a dict collects the parts' times (tools/detector_input_bench.py)"""
    import torch
    if phase_ms is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    phase_ms[name] = phase_ms.get(name, 0.0) + e0.elapsed_time(e1)


# ---------------------------------------------------------------------------------------------------------------- resize_images / resize_masks
def resize_images(images, shapes, flips=None, *, device=None, _phase_ms=None):
    """PIL's bilinear resize and the flip of a batch of images in one launch.  images: uint8 [H, W, 3] tensors (PIL's HWC layout), on the
    GPU or on the host -- small host ones go up with the tables, larger ones each in a copy of their own (_sources).  shapes[i]: (new_h, new_w); flips[i]: 0 / False (none),
    1 / True (horizontal), 2 (vertical); shapes may also hold draw_transforms' triples (flips=None).  Returns uint8 [3, new_h, new_w]
    tensors, planar: what copy_and_paste takes.  Inputs are not modified."""
    import torch
    what = "resize_images"
    if flips is not None and len(flips) != len(shapes):
        raise ValueError(f"{what}: {len(flips)} flips for {len(shapes)} shapes")
    transforms = _check_transforms(list(shapes) if flips is None else [(*s[:2], f) for s, f in zip(shapes, flips)], len(images), what)
    sizes = [_check_image(img, i, what) for i, img in enumerate(images)]
    dev = _device(images, device, what)
    B = len(images)
    if B == 0:
        return []
    tabs, pack = _Tables(), _Pack()
    desc, tiles, offs, out_bytes = _plan_images(tabs, sizes, transforms, what)
    where, hold = _sources(pack, images, dev)
    tab = tabs.array()
    o_desc, o_tab = pack.add(desc), pack.add(tab)
    with torch.cuda.device(dev):
        out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=dev)

        def fill(base):
            for i in range(B):
                desc[i, 0], desc[i, 1] = _addr(where[i], base), out.data_ptr() + offs[i]
        buf = pack.upload(dev, fill)
        _timed(lambda: _launch_bilinear(buf, o_desc, B, o_tab, tab.size, tiles), "resize", _phase_ms)
    del hold
    return [out[o:o + 3 * nh * nw].view(3, nh, nw) for o, (nh, nw, _) in zip(offs, transforms)]


def resize_masks(masks, shapes, flips=None, *, device=None, _phase_ms=None):
    """PIL's nearest resize and the flip of every instance mask of a batch in one launch.  masks[i]: bool or uint8 [N, H, W] (N may be 0;
    any non-zero value counts as set, so rle.decode's 0 / 255 output feeds it directly), on the GPU or on the host.  shapes / flips as in
    resize_images.  Returns (bool [N, new_h, new_w] tensors, bool [N] tensors: whether each resized mask has a set pixel), all on the
    device; nothing is read back."""
    import torch
    what = "resize_masks"
    if flips is not None and len(flips) != len(shapes):
        raise ValueError(f"{what}: {len(flips)} flips for {len(shapes)} shapes")
    transforms = _check_transforms(list(shapes) if flips is None else [(*s[:2], f) for s, f in zip(shapes, flips)], len(masks), what)
    mshapes = [_check_masks(m, i, what) for i, m in enumerate(masks)]
    dev = _device(masks, device, what)
    B = len(masks)
    if B == 0:
        return [], []
    tabs, pack = _Tables(), _Pack()
    desc, blocks, offs, out_bytes, flag0, n_flags = _plan_masks(tabs, mshapes, transforms, what)
    where, hold = _sources(pack, masks, dev)
    tab = tabs.array()
    o_desc, o_tab = pack.add(desc), pack.add(tab)
    with torch.cuda.device(dev):
        out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=dev)
        flags = torch.zeros(max(n_flags, 1), dtype=torch.int32, device=dev)

        def fill(base):
            for i, (N, H, W) in enumerate(mshapes):
                desc[i, 0], desc[i, 1], desc[i, 12] = _addr(where[i], base), out.data_ptr() + offs[i], H * W
        buf = pack.upload(dev, fill)
        _timed(lambda: _launch_nearest(buf, o_desc, B, o_tab, tab.size, blocks, flags), "masks", _phase_ms)
        res = [out[o:o + N * nh * nw].view(N, nh, nw).view(torch.bool) for o, (N, _, _), (nh, nw, _) in zip(offs, mshapes, transforms)]
        nonempty = [flags[f0:f0 + N] != 0 for f0, (N, _, _) in zip(flag0, mshapes)]
    del hold
    return res, nonempty


# ---------------------------------------------------------------------------------------------------------------- the mapper
def _rle_blob(recs):
    """umr_rle_decode's tables and characters for one mask per record, as rle.decode lays them out: (host u8 array, byte offsets of
    out_desc / group_start / seg_offsets / chars inside it, total characters, output bytes, output offset per record, largest mask)"""
    K = len(recs)
    nchars = np.array([len(c) for _, _, c in recs], dtype=np.int64)
    char_offsets = np.concatenate([[0], np.cumsum(nchars)]).astype(np.int64)
    out_desc = np.zeros((K, 3), dtype=np.int64)
    off = 0
    for g, (h, w, _) in enumerate(recs):
        out_desc[g] = (h, w, off)
        off += (h * w + 15) & ~15
    seg_offsets = np.zeros(K + 1, dtype=np.int64)
    gs = np.zeros((K + 2) & ~1, dtype=np.int32)
    gs[:K + 1] = np.arange(K + 1)
    tables = np.concatenate([char_offsets, out_desc.reshape(-1), seg_offsets, gs.view(np.int64)])
    o_desc, o_seg, o_gs, o_chars = (K + 1) * 8, (K + 1 + 3 * K) * 8, (K + 1 + 3 * K + K + 1) * 8, tables.size * 8
    host = np.concatenate([tables.view(np.uint8), np.frombuffer(b"".join(c for _, _, c in recs), dtype=np.uint8)])
    return host, (o_desc, o_gs, o_seg, o_chars), int(char_offsets[-1]), off, out_desc[:, 2].copy(), max(h * w for h, w, _ in recs)


def _read_annotations(annotations, i, H, W, what):
    """The non-crowd annotations of image i, checked: (source indices, float64 XYXY boxes [N,4], float32 scores [N], segmentations)"""
    import torch
    if not isinstance(annotations, (list, tuple)):
        raise ValueError(f"{what}: annotations[{i}] must be a list of dicts")
    src, boxes, scores, segs = [], [], [], []
    for a, obj in enumerate(annotations):
        tag = f"{what}: annotations[{i}][{a}]"
        if not isinstance(obj, dict):
            raise ValueError(f"{tag} must be a dict")
        if "keypoints" in obj:
            raise ValueError(f"{tag}: keypoints are not supported")
        if obj.get("iscrowd", 0) != 0:
            continue
        if "bbox" not in obj or "bbox_mode" not in obj:
            raise ValueError(f"{tag} needs 'bbox' and 'bbox_mode'")
        boxes.append(convert_box(obj["bbox"], obj["bbox_mode"], f"{tag}: bbox"))
        if "score" in obj:
            scores.append(float(obj["score"]))
        seg = obj.get("segmentation")
        if seg is None:
            raise ValueError(f"{tag} needs a 'segmentation' (a run-length record or a decoded [H, W] mask)")
        if isinstance(seg, (list, tuple)):
            raise ValueError(f"{tag}: segmentation is a polygon; under the 'bitmask' format the reference rasterises polygons after the "
                             "transform, which this module does not do (rle.from_polygons makes records of the untransformed ones)")
        if isinstance(seg, dict):
            if "size" not in seg or "counts" not in seg or len(seg["size"]) != 2:
                raise ValueError(f"{tag}: segmentation is not a run-length record {{'size': [H, W], 'counts': ...}}")
            if (int(seg["size"][0]), int(seg["size"][1])) != (H, W):
                raise ValueError(f"{tag}: segmentation has size {list(seg['size'])}, its image {[H, W]}")
        else:
            if isinstance(seg, np.ndarray):
                seg = torch.from_numpy(np.ascontiguousarray(seg))
            if not isinstance(seg, torch.Tensor) or seg.dtype not in (torch.bool, torch.uint8) or seg.dim() != 2:
                raise ValueError(f"{tag}: segmentation must be a run-length record or a bool / uint8 [H, W] mask")
            if tuple(seg.shape) != (H, W):
                raise ValueError(f"{tag}: segmentation has size {list(seg.shape)}, its image {[H, W]}")
        src.append(a)
        segs.append(seg)
    if scores and len(scores) != len(src):
        raise ValueError(f"{what}: annotations[{i}]: {len(scores)} of {len(src)} annotations carry a 'score'; all or none must")
    scores = np.asarray(scores, dtype=np.float32) if scores else np.ones(len(src), dtype=np.float32)
    return src, np.stack(boxes) if boxes else np.zeros((0, 4)), scores, segs


def map_batch(images, annotations=None, transforms=None, *, is_train=True, padded=False, min_size=MIN_SIZE_TRAIN, max_size=1333,
              sample_style="choice", flip="horizontal", np_random=np.random, image_ids=None, single_object_constraint=True, device=None,
              _phase_ms=None):
    """DatasetMapper.__call__ for a whole batch of decoded images.

    images: uint8 [H, W, 3] tensors, on the GPU or on the host.  annotations[i]: a list of dicts with `bbox`, `bbox_mode` (0 = XYXY_ABS,
    1 = XYWH_ABS), optional `score` and `iscrowd`, and `segmentation`: a run-length record, decoded on the device by rle.decode's kernels
    inside this call, or an already decoded bool / uint8 [H, W] mask (tensor on either side, or array).  Polygon segmentations, keypoints,
    `sem_seg` and precomputed proposals raise ValueError.  transforms: what draw_transforms returns; None draws now (min_size, max_size,
    sample_style, flip, np_random; the defaults are the recipe's).  image_ids: per image the dataset's `image_id` (is_single_object is
    true for a string that starts with "imagenet", when single_object_constraint is on).

    Returns one dict per image: `image` (uint8 [3, h, w]), `masks` (bool [M, h, w]), `boxes` (float32 [M, 4]), `scores` (float32 [M]),
    `classes` (int64 zeros), `source` (int64 [M]: the index of each instance's annotation in annotations[i]), `height`, `width`,
    `is_single_object`, all tensors on the device; directly valid as copy_and_paste items and as preprocess_image's input.  List
    form: the instances filter_empty_instances keeps, after the call's one device-to-host read (the non-empty flags and the run-length
    status words).  padded=True: no host read; every non-crowd instance is returned, with `keep` (bool [N] on the device) saying which
    ones the filter keeps, and a malformed run-length string gives an empty, dropped mask (`rle_status` says so: int32 per instance, 0
    for an instance that was not a record, None for an image without records; in
    list form it raises ValueError as rle.decode does).  is_train=False: no flip is drawn, annotations are ignored, and the dict holds
    `image` with the ORIGINAL `height` / `width`.  One host-to-device copy carries the tables, the boxes, the run-length strings and small
    host inputs; a large host image or mask stack goes up in a copy of its own (asynchronous from pinned memory).  Inputs are
    never modified; argument errors are ValueError before any launch."""
    import torch
    what = "map_batch"
    B = len(images)
    sizes = [_check_image(img, i, what) for i, img in enumerate(images)]
    if transforms is None:
        transforms = draw_transforms(sizes, min_size=min_size, max_size=max_size, sample_style=sample_style, flip=flip, is_train=is_train,
                                     np_random=np_random)
    transforms = _check_transforms(transforms, B, what)
    if image_ids is not None and len(image_ids) != B:
        raise ValueError(f"{what}: {len(image_ids)} image_ids for {B} images")
    if is_train:
        if annotations is None or len(annotations) != B:
            raise ValueError(f"{what}: {0 if annotations is None else len(annotations)} annotation lists for {B} images")
        for i, item in enumerate(annotations):
            if isinstance(item, dict):
                bad = [k for k in ("sem_seg", "sem_seg_file_name", "proposal_boxes", "proposals") if k in item]
                raise ValueError(f"{what}: annotations[{i}] must be the list of annotation dicts"
                                 + (f"; {bad[0]} is not supported" if bad else ""))
        notes = [_read_annotations(annotations[i], i, sizes[i][0], sizes[i][1], what) for i in range(B)]
    else:
        notes = [([], np.zeros((0, 4)), np.ones(0, dtype=np.float32), [])] * B
    seg_tensors = [s for n in notes for s in n[3] if not isinstance(s, dict)]
    dev = _device(list(images) + seg_tensors, device, what)
    if B == 0:
        return []
    from . import _lib as L
    from . import rle as R
    from ._tables import workspace
    from .ops import _p, _stream

    # ---- host: boxes, keep-by-box, tables, descriptors
    tabs, pack = _Tables(), _Pack()
    counts = [len(n[0]) for n in notes]
    boxes32 = [transform_boxes(n[1], H, W, nh, nw, f) for n, (H, W), (nh, nw, f) in zip(notes, sizes, transforms)]
    box_keep = [((b[:, 2] - b[:, 0]) > BOX_THRESHOLD) & ((b[:, 3] - b[:, 1]) > BOX_THRESHOLD) for b in boxes32]
    desc_i, tiles, offs_i, bytes_i = _plan_images(tabs, sizes, transforms, what)
    mshapes = [(c, H, W) for c, (H, W) in zip(counts, sizes)]
    desc_m, blocks, offs_m, bytes_m, flag0, n_flags = _plan_masks(tabs, mshapes, transforms, what)
    where_i, hold = _sources(pack, images, dev)
    # run-length records: all of the batch in one decode, in image order, so an image's masks lie one stride apart
    records = [s for n in notes for s in n[3] if isinstance(s, dict)]
    recs = R._prepare(records, None, 0, what)[0] if records else []
    K = len(recs)
    rle_host = rle_offs = None
    rle_bytes = 0
    if K:
        rle_host, rle_offs, total_chars, rle_bytes, rle_out_off, max_pixels = _rle_blob(recs)
        o_rle = pack.add(rle_host)
    # per image: where its masks come from
    mask_src, k = [], 0
    for i, n in enumerate(notes):
        segs = n[3]
        if not segs:
            mask_src.append(("none", 0, 0))
        elif all(isinstance(s, dict) for s in segs):
            mask_src.append(("rle", k, (sizes[i][0] * sizes[i][1] + 15) & ~15))
        elif all(not isinstance(s, dict) for s in segs) and _span(segs, *sizes[i]) is not None and \
                (segs[0].device.type != "cpu" or len(segs) * sizes[i][0] * sizes[i][1] >= DIRECT_BYTES):
            span = _span(segs, *sizes[i])                       # one tensor's slices: read in place, or sent up in one copy
            if span.device.type == "cpu":
                span = span.to(dev, non_blocking=True)
            hold.append(span)
            mask_src.append(("ptr", span.data_ptr(), span.stride(0)))
        elif all(not isinstance(s, dict) and s.device.type == "cpu" for s in segs) and \
                len(segs) * sizes[i][0] * sizes[i][1] < DIRECT_BYTES:                         # small and decoded on the host: they join the upload
            stacked = np.stack([s.numpy().view(np.uint8) if s.dtype == torch.bool else s.numpy() for s in segs])
            mask_src.append(("pack", pack.add(stacked), sizes[i][0] * sizes[i][1]))
        else:
            mask_src.append(("stack", k, sizes[i][0] * sizes[i][1]))
        k += sum(isinstance(s, dict) for s in segs)
    n_all = sum(counts)
    meta_boxes = np.concatenate(boxes32).astype(np.float32) if n_all else np.zeros((0, 4), np.float32)
    meta_scores = np.concatenate([n[2] for n in notes]).astype(np.float32) if n_all else np.zeros(0, np.float32)
    meta_src = np.concatenate([np.asarray(n[0], dtype=np.int64) for n in notes]) if n_all else np.zeros(0, np.int64)
    meta_keep = np.concatenate(box_keep).astype(np.int32) if n_all else np.zeros(0, np.int32)
    o_boxes, o_scores, o_src, o_bk = pack.add(meta_boxes), pack.add(meta_scores), pack.add(meta_src), pack.add(meta_keep)
    tab = tabs.array()
    o_di, o_dm, o_tab = pack.add(desc_i), pack.add(desc_m), pack.add(tab)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    with torch.cuda.device(dev):
        out = torch.empty(max(bytes_i + bytes_m, 16), dtype=torch.uint8, device=dev)
        # umr_rle_decode writes EVERY byte of every mask, zeros for a record with a non-zero status (csrc/rle_decode.hip,
        # rle_union_paint_kernel), so the buffer needs no clearing and a malformed record gives an empty mask
        rle_out = torch.empty(max(rle_bytes, 16), dtype=torch.uint8, device=dev)
        words = torch.zeros(max(K + n_flags, 1), dtype=torch.int32, device=dev)      # run-length status words | non-empty flags
        status, flags = words[:K], words[K:]
        # images whose segmentations are not all records: their masks are stacked here (decoded records are copied in after the decode)
        stacks = {}
        for i, (kind, k0, _) in enumerate(mask_src):
            if kind == "stack":
                stacks[i] = torch.empty((counts[i],) + sizes[i], dtype=torch.uint8, device=dev)

        def fill(base):
            for i in range(B):
                desc_i[i, 0], desc_i[i, 1] = _addr(where_i[i], base), out.data_ptr() + offs_i[i]
                kind, k0, stride = mask_src[i]
                src = {"none": lambda: 0, "rle": lambda: rle_out.data_ptr() + int(rle_out_off[k0]), "pack": lambda: base + k0, "ptr": lambda: k0,
                       "stack": lambda: stacks[i].data_ptr()}[kind]()
                desc_m[i, 0], desc_m[i, 1], desc_m[i, 12] = src, out.data_ptr() + bytes_i + offs_m[i], stride
        buf = pack.upload(dev, fill)                                                  # tables, boxes, strings and small inputs: one copy
        base = buf.data_ptr()
        vp = ctypes.c_void_p
        if K:
            nbytes = L.lib().umr_rle_decode_workspace(K, total_chars, 0, 0)
            ws = workspace(nbytes, dev)
            o_desc, o_gs, o_seg, o_chars = (o_rle + o for o in rle_offs)
            _timed(lambda: L.check(L.lib().umr_rle_decode(vp(base + o_chars), vp(base + o_rle), K, total_chars, vp(base + o_desc),
                                                          vp(base + o_gs), vp(base + o_seg), K, max_pixels, 0, _p(rle_out), rle_bytes, 255, 0,
                                                          _p(status), None, _p(ws), nbytes, _stream()), "umr_rle_decode"), "decode", _phase_ms)
        for i, st in stacks.items():                                                  # decoded masks that are not one tensor: a copy per mask
            k = mask_src[i][1]
            for j, s in enumerate(notes[i][3]):
                if isinstance(s, dict):
                    h, w, _ = recs[k]
                    st[j].copy_(rle_out[int(rle_out_off[k]):int(rle_out_off[k]) + h * w].view(h, w))
                    k += 1
                else:
                    st[j].copy_(s.view(torch.uint8) if s.dtype == torch.bool else s, non_blocking=True)
        _timed(lambda: _launch_bilinear(buf, o_di, B, o_tab, tab.size, tiles), "resize", _phase_ms)
        if blocks:
            _timed(lambda: _launch_nearest(buf, o_dm, B, o_tab, tab.size, blocks, flags), "masks", _phase_ms)
        del hold

        imgs = [out[o:o + 3 * nh * nw].view(3, nh, nw) for o, (nh, nw, _) in zip(offs_i, transforms)]
        if not is_train:
            return [{"image": imgs[i], "height": sizes[i][0], "width": sizes[i][1]} for i in range(B)]
        masks = [out[bytes_i + o:bytes_i + o + c * nh * nw].view(c, nh, nw).view(torch.bool)
                 for o, c, (nh, nw, _) in zip(offs_m, counts, transforms)]
        boxes_d = buf[o_boxes:o_boxes + n_all * 16].view(torch.float32).view(n_all, 4)
        scores_d = buf[o_scores:o_scores + n_all * 4].view(torch.float32)
        src_d = buf[o_src:o_src + n_all * 8].view(torch.int64)
        bk_d = buf[o_bk:o_bk + n_all * 4].view(torch.int32)
        classes_d = torch.zeros(n_all, dtype=torch.int64, device=dev)

        def single(i):
            iid = None if image_ids is None else image_ids[i]
            return bool(isinstance(iid, str) and iid.startswith("imagenet") and single_object_constraint)

        def item(i, sel=None):
            a, b = int(first[i]), int(first[i + 1])
            pick = (lambda t: t[a:b]) if sel is None else (lambda t: t[a:b][sel])
            return {"image": imgs[i], "masks": masks[i] if sel is None else masks[i][sel], "boxes": pick(boxes_d), "scores": pick(scores_d),
                    "classes": pick(classes_d), "source": pick(src_d), "height": transforms[i][0], "width": transforms[i][1],
                    "is_single_object": single(i)}
        if padded:
            keep_d = (flags[:n_all] != 0) & (bk_d != 0)
            res = []
            for i in range(B):
                a, b = int(first[i]), int(first[i + 1])
                d = item(i)
                d["keep"] = keep_d[a:b]
                kind, k0, _ = mask_src[i]
                d["rle_status"] = status[k0:k0 + counts[i]] if kind == "rle" else None
                if kind == "stack" and any(isinstance(s, dict) for s in notes[i][3]):     # records among decoded masks: their words, 0 elsewhere
                    d["rle_status"] = torch.zeros(counts[i], dtype=torch.int32, device=dev)
                    for j, s in enumerate(notes[i][3]):
                        if isinstance(s, dict):
                            d["rle_status"][j:j + 1].copy_(status[k0:k0 + 1])
                            k0 += 1
                res.append(d)
            return res
        words_h = words.cpu().numpy() if K + n_all else np.zeros(0, np.int32)         # the call's only device-to-host read
        st_h, fl_h = words_h[:K], words_h[K:K + n_all]
        bad = np.flatnonzero(st_h)
        if bad.size:
            kb = int(bad[0])
            why = "; ".join(t for bit, t in R._STATUS_BITS if int(st_h[kb]) & bit)
            raise ValueError(f"{what}: run-length record {kb} of the batch is not a run-length string of a {recs[kb][0]}x{recs[kb][1]} "
                             f"mask: {why}")
        keep_h = (fl_h != 0) & (meta_keep != 0)
        sels, parts, n_idx = [None] * B, [], 0
        for i in range(B):
            a, b = int(first[i]), int(first[i + 1])
            if not keep_h[a:b].all():
                idx = np.flatnonzero(keep_h[a:b]).astype(np.int64)
                sels[i] = (n_idx, idx.size)
                parts.append(idx)
                n_idx += idx.size
        idx_d = torch.from_numpy(np.concatenate(parts)).to(dev) if parts else None
        return [item(i, None if sels[i] is None else idx_d[sels[i][0]:sels[i][0] + sels[i][1]]) for i in range(B)]


# ---------------------------------------------------------------------------------------------------------------- preprocess_image
def preprocess_image(items_or_images, pixel_mean, pixel_std, size_divisibility=32, pad_value=0.0, *, _phase_ms=None):
    """GeneralizedRCNN.preprocess_image: normalise, pad and batch in one launch.  items_or_images: map_batch's or copy_and_paste's outputs
    (dicts with `image`) or bare uint8 [3, h, w] tensors, on the GPU.  pixel_mean / pixel_std: three values each, rounded to float32 as
    the model's buffers are.  Returns (float32 [B, 3, Hp, Wp], image_sizes = [(h, w)]): (float32(u8) - mean[c]) / std[c] at the top
    left, pad_value elsewhere; Hp, Wp are the batch maxima, rounded up to size_divisibility when it is > 1 (32 for the FPN)."""
    import torch
    what = "preprocess_image"
    images = [it["image"] if isinstance(it, dict) else it for it in items_or_images]
    mean, std = np.asarray(pixel_mean, dtype=np.float32).reshape(-1), np.asarray(pixel_std, dtype=np.float32).reshape(-1)
    if mean.size != 3 or std.size != 3:
        raise ValueError(f"{what}: pixel_mean and pixel_std must hold three values each")
    if not np.isfinite(mean).all() or not np.isfinite(std).all() or (std == 0).any():
        raise ValueError(f"{what}: pixel_mean must be finite, pixel_std finite and non-zero")
    size_divisibility = int(size_divisibility)
    if size_divisibility < 0:
        raise ValueError(f"{what}: size_divisibility must not be negative")
    if not images:
        raise ValueError(f"{what}: an empty batch")
    sizes = []
    for i, img in enumerate(images):
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[0] != 3 or img.shape[1] < 1 or \
                img.shape[2] < 1:
            got = f"{img.dtype} {list(img.shape)}" if isinstance(img, torch.Tensor) else type(img).__name__
            raise ValueError(f"{what}: images[{i}] must be a uint8 [3, h, w] tensor, got {got}")
        sizes.append((int(img.shape[1]), int(img.shape[2])))
    devs = {img.device for img in images}
    if any(d.type != "cuda" for d in devs):
        raise RuntimeError(f"unmore_amd.detector_input.{what} runs on the MI355X only (no CPU fallback); tests/det_input_common.py restates "
                           "it on the host")
    if len(devs) > 1:
        raise ValueError(f"{what}: every image must be on the same device, got {sorted(str(d) for d in devs)}")
    dev = devs.pop()
    Hp, Wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if size_divisibility > 1:
        Hp = (Hp + size_divisibility - 1) // size_divisibility * size_divisibility
        Wp = (Wp + size_divisibility - 1) // size_divisibility * size_divisibility
    B = len(images)
    if B * 3 * Hp * Wp >= 1 << 40 or Hp >= 1 << 30 or Wp >= 1 << 30:
        raise ValueError(f"{what}: a batch of {B} x 3 x {Hp} x {Wp} is too large")
    from . import _lib as L
    from .ops import _p, _stream
    hold = [img.contiguous() for img in images]
    desc = np.zeros((B, _NP), dtype=np.int64)
    for i, (img, (h, w)) in enumerate(zip(hold, sizes)):
        desc[i] = (img.data_ptr(), h, w, 0)
    with torch.cuda.device(dev):
        d = torch.from_numpy(desc).to(dev)
        out = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=dev)
        _timed(lambda: L.check(L.lib().umr_det_normalize_pad(_p(d), B, Hp, Wp, float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]),
                                                             float(std[1]), float(std[2]), float(np.float32(pad_value)), _p(out), _stream()),
                               "umr_det_normalize_pad"), "normalise", _phase_ms)
    del hold
    return out, sizes
