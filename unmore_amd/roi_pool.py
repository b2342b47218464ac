"""Detectron2's ROIPooler on the device (detectron2.modeling.poolers.ROIPooler with pooler_type "ROIAlignV2", which the stage-3 detector
builds at cad/modeling/roi_heads/custom_cascade_rcnn.py:117-122 and roi_heads.py:674-679, 709-716 and calls once per cascade stage and
once for the mask head): `assign_boxes_to_levels`, `roi_align` (torchvision's rule, aligned=True) and the `ROIPooler` module, all over
csrc/roi_pool.hip.  One small launch writes (image, level) per box, one launch pools every box of every level and image -- the
reference's per-level nonzero / index / roi_align / index_put and its host synchronisation are gone -- and the backward writes the
gradient of every feature map in one launch without float atomics: the same input gives the same bytes on every run.  The level
descriptors travel in the kernel's arguments, so nothing but the N + 1 box counts is uploaded and nothing is read back.  No CPU fallback: tests/roi_pool_common.py restates the method in NumPy.

Departures from Detectron2 / torchvision, all on inputs they leave undefined or fault on:
  * a box with a coordinate that is not finite or beyond +-2^20 (mask_loss's bound) gives a zero row; it is assigned level 0 and adds
    nothing to the gradient (roi_align: likewise a roi whose image index is not an integer in [0, N));
  * a box with roi <= 0 on an axis gives zeros (torchvision averages an empty grid); a box of negative area, whose level is NaN in the
    original, is assigned level 0 (and pools to zeros by the line above);
  * a tap whose summed weight is exactly 0 adds 0 whatever the map holds there, so a NaN spreads only to the bins that weigh it.
Only aligned=True / "ROIAlignV2" is implemented; the output side is at most 64, the sampling ratio at most 1024, a scale at most 16."""
import ctypes
import math
import struct

import torch

from . import _lib as L
from . import _tables as T
from .ops import _p, _stream

MAX_LEVELS = 8
MAX_SIDE = 64
MAX_SAMPLING_RATIO = 1024
MAX_SCALE = 16.0
MAX_LDS_BYTES = 64 * 1024


def _lds_bytes(side, max_h, max_w):
    return 4 * (max_h + max_w) + 64 * side + 1112         # csrc/roi_pool.hip: rp_lds_bytes


def _device(tensors, what):
    return T.one_device(tensors, "roi_pool", what, " (roi_align_np, pooler_np)")


def _check_side(output_size):
    if isinstance(output_size, (tuple, list)) and len(output_size) == 2 and output_size[0] == output_size[1]:
        output_size = output_size[0]
    if not isinstance(output_size, int) or isinstance(output_size, bool) or not 1 <= output_size <= MAX_SIDE:
        raise ValueError(f"roi_pool: output_size must be an integer (or a square pair) in [1, {MAX_SIDE}], got {output_size!r}")
    return output_size


def _check_ratio(sampling_ratio):
    if not isinstance(sampling_ratio, int) or isinstance(sampling_ratio, bool) or not 0 <= sampling_ratio <= MAX_SAMPLING_RATIO:
        raise ValueError(f"roi_pool: sampling_ratio must be an integer in [0, {MAX_SAMPLING_RATIO}], got {sampling_ratio!r}")
    return sampling_ratio


def _check_features(feats, side):
    """shape and dtype checks of the level maps, without touching their data: (N, C)"""
    for k, f in enumerate(feats):
        if not isinstance(f, torch.Tensor) or f.dim() != 4 or f.dtype not in (torch.float32, torch.bfloat16) or min(f.shape) < 1:
            raise ValueError(f"roi_pool: features[{k}] must be float32 or bfloat16 [N, C, H, W] with no empty dimension, got "
                             f"{getattr(f, 'dtype', type(f))} {list(getattr(f, 'shape', []))}")
        if f.shape[:2] != feats[0].shape[:2] or f.dtype != feats[0].dtype:
            raise ValueError(f"roi_pool: features[{k}] is {f.dtype} {list(f.shape)}, features[0] is {feats[0].dtype} {list(feats[0].shape)}: "
                             "every level has the same N, C and type")
        if f.shape[2] * f.shape[3] >= 1 << 31:
            raise ValueError(f"roi_pool: features[{k}]: a map of 2^31 pixels or more")
    max_h, max_w = max(int(f.shape[2]) for f in feats), max(int(f.shape[3]) for f in feats)
    if _lds_bytes(side, max_h, max_w) > MAX_LDS_BYTES:
        raise ValueError(f"roi_pool: the axis tables of a {max_h} x {max_w} map at side {side} take {_lds_bytes(side, max_h, max_w)} bytes "
                         f"of LDS, more than {MAX_LDS_BYTES}")
    return int(feats[0].shape[0]), int(feats[0].shape[1])


def _check_boxes(b, what, cols=4):
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or b.dim() != 2 or b.shape[1] != cols:
        raise ValueError(f"roi_pool: {what} must be float32 [R, {cols}], got {getattr(b, 'dtype', type(b))} {list(getattr(b, 'shape', []))}")
    return int(b.shape[0])


def _level_table(tensors, sizes, scales):
    """the host array of csrc/roi_pool.hip: per level the map's pointer (0 for None), H, W and the bits of the float32 scale"""
    tab = (ctypes.c_int64 * (4 * len(scales)))()
    for k, (t, (h, w), s) in enumerate(zip(tensors, sizes, scales)):
        tab[4 * k], tab[4 * k + 1], tab[4 * k + 2] = (0 if t is None else t.data_ptr()), h, w
        tab[4 * k + 3] = struct.unpack("<I", struct.pack("<f", s))[0]
    return tab


def _prepare(boxes, first, N, n_levels, min_level, max_level, canonical_box_size, canonical_level):
    """info int32 [R,2] = (image, level) per row of boxes ([R,4] with first, or [R,5] rois)"""
    R = int(boxes.shape[0])
    info = torch.empty((R, 2), dtype=torch.int32, device=boxes.device)
    if R:
        L.check(L.lib().umr_roi_pool_prepare(_p(boxes), int(boxes.shape[1]), R, _p(first), N, n_levels, min_level, max_level,
                                             float(canonical_box_size), int(canonical_level), _p(info), _stream()), "umr_roi_pool_prepare")
    return info


class _Pool(torch.autograd.Function):
    """out [R,C,P,P] of boxes / info over the level maps; cfg = (scales, side, sampling_ratio, first, _phase_ms)"""

    @staticmethod
    def forward(ctx, boxes, info, cfg, *feats):
        scales, side, ratio, first, phase_ms = cfg
        maps = [f.detach().contiguous() for f in feats]
        N, C, R = int(maps[0].shape[0]), int(maps[0].shape[1]), int(boxes.shape[0])
        out = torch.empty((R, C, side, side), dtype=maps[0].dtype, device=maps[0].device)
        tab = _level_table(maps, [m.shape[2:] for m in maps], scales)

        def launch(_):
            L.check(L.lib().umr_roi_pool_forward(tab, len(maps), N, C, T.dtype_code(maps[0]), _p(boxes), int(boxes.shape[1]), _p(info), R,
                                                 side, ratio, _p(out), _stream()), "umr_roi_pool_forward")
        T.timed(launch, (("forward", 1),), phase_ms)
        ctx.save_for_backward(boxes, info, first)
        ctx.cfg = (scales, side, ratio, phase_ms, [tuple(m.shape) for m in maps], maps[0].dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        boxes, info, first = ctx.saved_tensors
        scales, side, ratio, phase_ms, shapes, dtype = ctx.cfg
        g = grad_out.detach().to(dtype).contiguous()
        need = ctx.needs_input_grad[3:]
        grads = [torch.empty(s, dtype=dtype, device=g.device) if n else None for s, n in zip(shapes, need)]
        N, C, R = shapes[0][0], shapes[0][1], int(boxes.shape[0])
        tab = _level_table(grads, [s[2:] for s in shapes], scales)

        def launch(_):
            L.check(L.lib().umr_roi_pool_backward(tab, len(shapes), N, C, L.BF16 if dtype == torch.bfloat16 else L.F32, _p(boxes),
                                                  int(boxes.shape[1]), _p(info), _p(first), R, side, ratio, _p(g), _stream()),
                    "umr_roi_pool_backward")
        with torch.cuda.device(g.device):
            T.timed(launch, (("backward", 1),), phase_ms)
        return (None, None, None) + tuple(grads)


def assign_boxes_to_levels(box_lists, min_level, max_level, canonical_box_size=224, canonical_level=4):
    """Detectron2's assign_boxes_to_levels on the device: int64 [R] level indices in [0, max_level - min_level].

    box_lists: float32 [R,4] XYXY, or a list of such tensors / objects with `.tensor` (concatenated in order).  The float32 sequence of
    the original, operation by operation: floor(canonical_level + log2(sqrt(area) / canonical_box_size + 1e-8)) clamped to
    [min_level, max_level], minus min_level.  A box the device refuses (see the module's departures) and a box of negative area get
    level 0.  ValueError for argument errors before any launch, RuntimeError off the GPU."""
    boxes = [T.unwrap(b) for b in box_lists] if isinstance(box_lists, (list, tuple)) else [T.unwrap(box_lists)]
    for k, b in enumerate(boxes):
        _check_boxes(b, f"boxes[{k}]")
    n_levels = _check_level_range(min_level, max_level, canonical_box_size, canonical_level)
    if not boxes:
        raise ValueError("roi_pool: no boxes")
    dev = _device(boxes, "assign_boxes_to_levels")
    with torch.cuda.device(dev):
        cat = torch.cat(boxes).contiguous()
        first = torch.tensor([0, cat.shape[0]], dtype=torch.int32).to(dev)
        info = _prepare(cat, first, 1, n_levels, min_level, max_level, canonical_box_size, canonical_level)
    return info[:, 1].to(torch.int64)


def _check_level_range(min_level, max_level, canonical_box_size, canonical_level):
    for name, v in (("min_level", min_level), ("max_level", max_level), ("canonical_level", canonical_level)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError(f"roi_pool: {name} must be an integer, got {v!r}")
    if not 0 <= min_level <= max_level or max_level - min_level + 1 > MAX_LEVELS:
        raise ValueError(f"roi_pool: 0 <= min_level <= max_level and at most {MAX_LEVELS} levels, got {min_level}, {max_level}")
    if not canonical_box_size > 0:
        raise ValueError(f"roi_pool: canonical_box_size must be positive, got {canonical_box_size!r}")
    return max_level - min_level + 1


def roi_align(features, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True, *, _phase_ms=None):
    """torchvision.ops.roi_align(features, rois, output_size, spatial_scale, sampling_ratio, aligned=True) on the device.

    features: float32 or bfloat16 [N,C,H,W]; rois: float32 [R,5] = (image index, x1, y1, x2, y2); returns [R,C,P,P] in the features' type,
    differentiable with respect to the features (not the rois).  Arithmetic and sums in float32: start = lo * scale - .5,
    roi = (hi * scale - .5) - start, bin = roi / P, grid = sampling_ratio or ceil(bin) when it is 0, a sample at
    start + p * bin + (i + .5) * bin / grid adds 0 outside [-1, size], else is clamped to [0, size - 1] and read bilinearly; the bin is the
    mean over grid_h * grid_w.  Any footprint and any grid are accepted.  The module's docstring lists the departures.  R == 0 returns an
    empty tensor without a launch.  ValueError for argument errors before any launch, RuntimeError off the GPU."""
    if not aligned:
        raise ValueError("roi_pool: only aligned=True (Detectron2's ROIAlignV2) is implemented")
    side, ratio = _check_side(output_size), _check_ratio(sampling_ratio)
    N, C = _check_features([features], side)
    R = _check_boxes(rois, "rois", 5)
    scale = float(spatial_scale)
    if not 0 < scale <= MAX_SCALE:
        raise ValueError(f"roi_pool: spatial_scale must be in (0, {MAX_SCALE}], got {spatial_scale!r}")
    dev = _device([features, rois], "roi_align")
    if R == 0:
        return features.new_zeros((0, C, side, side))
    with torch.cuda.device(dev):
        rois = rois.detach().contiguous()
        info = _prepare(rois, None, N, 1, 0, 0, 224, 4)
        return _Pool.apply(rois, info, ((scale,), side, ratio, None, _phase_ms), features)


class ROIPooler(torch.nn.Module):
    """detectron2.modeling.poolers.ROIPooler(output_size, scales, sampling_ratio, pooler_type, canonical_box_size, canonical_level) for
    pooler_type "ROIAlignV2".

    scales: the maps' scales against the frame, consecutive powers of two (1/4, 1/8, ...); min_level = -log2(scales[0]) and max_level =
    -log2(scales[-1]) as in the original.  forward(x, box_lists): x a list of [N,C,H_l,W_l] maps (float32 or bfloat16), one per scale;
    box_lists one float32 [R_k,4] XYXY tensor (or object with `.tensor`) per image, an image without boxes included.  Returns
    [sum R_k, C, P, P] in the maps' type and in input box order, differentiable with respect to every x[l].  A single level skips the
    assignment, as the original does.  The module's docstring lists the departures."""

    def __init__(self, output_size, scales, sampling_ratio=0, pooler_type="ROIAlignV2", canonical_box_size=224, canonical_level=4):
        super().__init__()
        if pooler_type != "ROIAlignV2":
            raise ValueError(f"roi_pool: unknown pooler_type {pooler_type!r}: only 'ROIAlignV2' is implemented")
        self.output_size = _check_side(output_size)
        self.sampling_ratio = _check_ratio(sampling_ratio)
        scales = [float(s) for s in scales]
        if not scales or len(scales) > MAX_LEVELS or not all(0 < s <= MAX_SCALE for s in scales):
            raise ValueError(f"roi_pool: 1 to {MAX_LEVELS} scales in (0, {MAX_SCALE}], got {scales}")
        lo, hi = -math.log2(scales[0]), -math.log2(scales[-1])
        if not (math.isclose(lo, round(lo)) and math.isclose(hi, round(hi))):
            raise ValueError(f"roi_pool: featuremap scales must be powers of two, got {scales}")
        self.min_level, self.max_level = int(round(lo)), int(round(hi))
        if len(scales) != self.max_level - self.min_level + 1 or any(s != 2.0 ** -(self.min_level + k) for k, s in enumerate(scales)):
            raise ValueError(f"roi_pool: the scales must be consecutive powers of two, got {scales}")
        _check_level_range(self.min_level, self.max_level, canonical_box_size, canonical_level)
        self.scales = tuple(scales)
        self.canonical_box_size, self.canonical_level = canonical_box_size, canonical_level

    def forward(self, x, box_lists, *, _phase_ms=None):
        if not isinstance(x, (list, tuple)) or not isinstance(box_lists, (list, tuple)):
            raise ValueError("roi_pool: ROIPooler takes a list of level maps and a list of boxes per image")
        if len(x) != len(self.scales):
            raise ValueError(f"roi_pool: {len(x)} level maps for {len(self.scales)} scales")
        N, C = _check_features(x, self.output_size)
        boxes = [T.unwrap(b) for b in box_lists]
        if len(boxes) != N:
            raise ValueError(f"roi_pool: {len(boxes)} box lists for {N} images")
        counts = [_check_boxes(b, f"box_lists[{k}]") for k, b in enumerate(boxes)]
        if sum(counts) >= 1 << 31:
            raise ValueError("roi_pool: 2^31 boxes or more")
        dev = _device(list(x) + boxes, "ROIPooler")
        side = self.output_size
        if sum(counts) == 0:
            return x[0].new_zeros((0, C, side, side))
        prefix = [0]
        for n in counts:
            prefix.append(prefix[-1] + n)
        with torch.cuda.device(dev):
            cat = torch.cat([b.detach() for b in boxes]).contiguous()
            first = torch.tensor(prefix, dtype=torch.int32).to(dev)
            info = _prepare(cat, first, N, len(self.scales), self.min_level, self.max_level, self.canonical_box_size, self.canonical_level)
            return _Pool.apply(cat, info, (self.scales, side, self.sampling_ratio, first, _phase_ms), *x)
