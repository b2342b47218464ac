"""The network of the stage-3 detector's RPN on the device, and the proposal generator as one module: Detectron2's StandardRPNHead (a
3x3 convolution with ReLU, the 1x1 `objectness_logits` (A channels) and `anchor_deltas` (4A channels) convolutions, the same weights on
p2..p6) and RPN.forward (cad/modeling/meta_arch/rcnn.py:165, 213, 333: self.proposal_generator(images, features, gt_instances)).

  predict / predict_bwd   the two predictors and their backward on the hidden map T [M, C] of ALL levels stacked (NHWC rows, level after
                          level), written to / read from the per-level NCHW maps that rpn.rpn_proposals and rpn_loss.rpn_losses take in
                          place: one launch each whatever the number of levels, plus the finishing sum (csrc/rpn_head.hip)
  StandardRPNHead         the parameters under Detectron2's names and forward(features) as ONE autograd Function: NCHW -> NHWC, per level
                          the library's implicit-GEMM convolution into a slice of T, one predict launch; backward: one predict_bwd launch
                          (+ finish), per level the convolution's weight gradient accumulated into one buffer and its data gradient
  RPN                     head -> (training) rpn_loss.label_and_sample_anchors + rpn_losses -> rpn.rpn_proposals on the detached outputs

Activations are stored in the compute type as the GEMM rounds them, and the predictors read those stored values: forward and backward
see the same ReLU mask.  predict_bwd writes its gradient OVER T, so the backward runs once per forward and raises otherwise.  With a
bfloat16 compute type the incoming gradients are rounded to bfloat16 for the matrix cores (csrc/rpn_head.hip, "Rounding").

Limits (ValueError before any launch): A <= 3 (5A <= 16), box dimension 4, C a multiple of 64 up to 1024, at most 8 levels, M < 2^31.
No CPU fallback: tests/rpn_head_common.py restates the head in float64."""
import ctypes

import torch

from . import _conv_head as H
from . import _lib as L
from . import _tables as T
from . import ops, packs, rpn, rpn_loss
from .ops import _p, _stream

MAX_CHANNELS = H.MAX_CHANNELS
MAX_ANCHORS = 3              # 5A <= 16: one matrix-core tile (csrc/rpn_head.hip: RH_MAX_A)
MAX_LEVELS = rpn.MAX_LEVELS
_DTYPES = H.DTYPES


def _check_shape(C, A, what):
    H.check_channels(C, f"rpn_head: {what}: C")
    if not isinstance(A, int) or isinstance(A, bool) or not 1 <= A <= MAX_ANCHORS:
        raise ValueError(f"rpn_head: {what}: between 1 and {MAX_ANCHORS} anchors per position (5A <= 16), got {A!r}")


def _check_tail(Tm, sizes, N, weights, what):
    """(C, A, M, first rows) of the checked arguments of predict / predict_bwd; weights = (wo, bo or None, wd, bd or None)"""
    if not isinstance(Tm, torch.Tensor) or Tm.dtype not in _DTYPES or Tm.dim() != 2 or not Tm.is_contiguous():
        raise ValueError(f"rpn_head: {what}: T must be contiguous float32 or bfloat16 [M, C], got {getattr(Tm, 'dtype', type(Tm))} "
                         f"{list(getattr(Tm, 'shape', []))}")
    wo, bo, wd, bd = weights
    if not isinstance(wo, torch.Tensor) or wo.dim() < 2:
        raise ValueError(f"rpn_head: {what}: wo must be float32 [A, C]")
    C, A = int(Tm.shape[1]), int(wo.shape[0])
    _check_shape(C, A, what)
    for t, shape, name in ((wo, (A, C), "wo"), (bo, (A,), "bo"), (wd, (4 * A, C), "wd"), (bd, (4 * A,), "bd")):
        if t is None and name in ("bo", "bd"):
            continue
        n = 1
        for s in shape:
            n *= s
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != n or t.shape[0] != shape[0] or not t.is_contiguous():
            raise ValueError(f"rpn_head: {what}: {name} must be contiguous float32 {list(shape)}, got {getattr(t, 'dtype', type(t))} "
                             f"{list(getattr(t, 'shape', []))}")
    if not isinstance(N, int) or isinstance(N, bool) or N < 0:
        raise ValueError(f"rpn_head: {what}: N must be a non-negative integer, got {N!r}")
    if not isinstance(sizes, (list, tuple)) or not 1 <= len(sizes) <= MAX_LEVELS:
        raise ValueError(f"rpn_head: {what}: between 1 and {MAX_LEVELS} levels of (H, W), got {sizes!r}")
    first, M = [], 0
    for k, hw in enumerate(sizes):
        try:
            h, w = hw
        except (TypeError, ValueError):
            raise ValueError(f"rpn_head: {what}: sizes[{k}] must be (H, W), got {hw!r}") from None
        rpn._int(h, f"sizes[{k}][0]", 1), rpn._int(w, f"sizes[{k}][1]", 1)
        first.append(M)
        M += N * int(h) * int(w)
    if M >= 1 << 31:
        raise ValueError(f"rpn_head: {what}: M = {M}, 2^31 or more")
    if int(Tm.shape[0]) != M:
        raise ValueError(f"rpn_head: {what}: T has {int(Tm.shape[0])} rows, the levels {M}")
    return C, A, M, first


def _level_table(sizes, first_maps, second_maps):
    tab = (ctypes.c_int64 * (4 * len(sizes)))()
    for k, ((h, w), a, b) in enumerate(zip(sizes, first_maps, second_maps)):
        tab[4 * k:4 * k + 4] = [int(h), int(w), a.data_ptr(), b.data_ptr()]
    return tab


def predict(Tm, sizes, N, wo, bo, wd, bd, *, out_f32=False):
    """The two predictors on the stacked hidden map (include/umr.h, umr_rpn_head_predict): Tm [M, C] float32 or bfloat16, level l's rows
    from N * sum of the earlier H * W, row (n * H_l + y) * W_l + x; sizes: (H, W) per level; wo [A, C] (or [A, C, 1, 1]), bo [A],
    wd [4A, C], bd [4A] float32.  Returns (logits, deltas): lists of [N, A, H_l, W_l] and [N, 4A, H_l, W_l] in Tm's type (float32 with
    out_f32), one launch.  Tm is only read."""
    C, A, M, _ = _check_tail(Tm, sizes, N, (wo, bo, wd, bd), "predict")
    dev = T.one_device([Tm, wo, bo, wd, bd], "rpn_head", "predict")
    odt = torch.float32 if out_f32 else Tm.dtype
    with torch.cuda.device(dev):
        logits = [torch.empty((N, A, int(h), int(w)), dtype=odt, device=dev) for h, w in sizes]
        deltas = [torch.empty((N, 4 * A, int(h), int(w)), dtype=odt, device=dev) for h, w in sizes]
        tab = _level_table(sizes, logits, deltas)
        L.check(L.lib().umr_rpn_head_predict(_p(Tm), tab, len(sizes), N, C, A, _p(wo), _p(bo), _p(wd), _p(bd), T.dtype_code(Tm),
                                             int(bool(out_f32)), _stream()), "umr_rpn_head_predict")
    return logits, deltas


def predict_bwd(Tm, sizes, N, dlogits, ddeltas, wo, wd, *, _phase_ms=None):
    """The predictors' backward and the ReLU mask of the hidden map in one pass over Tm (umr_rpn_head_predict_bwd): Tm is OVERWRITTEN
    with G = (T > 0) * sum_j g[m, j] w[j, c], rounded once to Tm's type.  dlogits / ddeltas: lists of contiguous [N, A, H_l, W_l] /
    [N, 4A, H_l, W_l] maps, all in Tm's type or all float32.  Returns (G -- Tm itself --, dwo [A, C], dbo [A], dwd [4A, C], dbd [4A])
    float32; the sums go through per-workgroup partials added in a fixed order, so the same input gives the same bytes."""
    C, A, M, _ = _check_tail(Tm, sizes, N, (wo, None, wd, None), "predict_bwd")
    if not isinstance(dlogits, (list, tuple)) or not isinstance(ddeltas, (list, tuple)) or len(dlogits) != len(sizes) or \
            len(ddeltas) != len(sizes):
        raise ValueError(f"rpn_head: predict_bwd: dlogits and ddeltas are lists with one map per level, {len(sizes)} of them")
    maps = list(dlogits) + list(ddeltas)
    for k, g in enumerate(maps):
        h, w = sizes[k % len(sizes)]
        shape = (N, A if k < len(sizes) else 4 * A, int(h), int(w))
        if not isinstance(g, torch.Tensor) or tuple(g.shape) != shape or not g.is_contiguous() or g.dtype not in (Tm.dtype, torch.float32) \
                or g.dtype != maps[0].dtype:
            raise ValueError(f"rpn_head: predict_bwd: gradient map {k} must be contiguous {list(shape)}, all in T's type or all float32, got "
                             f"{getattr(g, 'dtype', type(g))} {list(getattr(g, 'shape', []))}")
    dev = T.one_device([Tm, wo, wd] + maps, "rpn_head", "predict_bwd")
    with torch.cuda.device(dev):
        dwo, dbo = torch.empty((A, C), dtype=torch.float32, device=dev), torch.empty(A, dtype=torch.float32, device=dev)
        dwd, dbd = torch.empty((4 * A, C), dtype=torch.float32, device=dev), torch.empty(4 * A, dtype=torch.float32, device=dev)
        nbytes = L.lib().umr_rpn_head_workspace(M, C, A)
        ws = T.workspace(nbytes, dev)
        tab = _level_table(sizes, dlogits, ddeltas)

        def launch(phases):
            L.check(L.lib().umr_rpn_head_predict_bwd(_p(Tm), tab, len(sizes), N, C, A, int(maps[0].dtype == torch.float32), _p(wo), _p(wd),
                                                     _p(dwo), _p(dbo), _p(dwd), _p(dbd), _p(ws), nbytes, T.dtype_code(Tm), phases,
                                                     _stream()), "umr_rpn_head_predict_bwd")
        T.timed(launch, (("predict_bwd", 1), ("predict_finish", 2)), _phase_ms)
    return Tm, dwo, dbo, dwd, dbd


def _is_nhwc(f, dt):
    return f.dtype == dt and f.permute(0, 2, 3, 1).is_contiguous()


class _Head(torch.autograd.Function):
    """(logits of every level, deltas of every level) of (cfg, *features, *parameters); cfg = (head, compute dtype, _keep, _marks)"""

    @staticmethod
    def forward(ctx, cfg, *args):
        head, dt, keep, marks = cfg
        nl = len(args) - 6
        feats, params = args[:nl], args[nl:]
        cw, cb, wo, bo, wd, bd = params
        N, C, A = int(feats[0].shape[0]), head.in_channels, head.num_anchors
        dev = feats[0].device
        sizes = [(int(f.shape[2]), int(f.shape[3])) for f in feats]
        live = [k for k, (h, w) in enumerate(sizes) if N * h * w > 0]
        ctx.cfg, ctx.nl, ctx.N, ctx.sizes, ctx.live, ctx.done = cfg, nl, N, sizes, live, False
        ctx.f_dtypes = [f.dtype for f in feats]
        logits = [torch.empty((N, A, h, w), dtype=dt, device=dev) for h, w in sizes]
        deltas = [torch.empty((N, 4 * A, h, w), dtype=dt, device=dev) for h, w in sizes]
        if not live:
            ctx.save_for_backward(*params)
            return tuple(logits + deltas)
        lsizes = [sizes[k] for k in live]
        first, M = [], 0
        for h, w in lsizes:
            first.append(M)
            M += N * h * w
        with torch.cuda.device(dev):
            H.mark(marks, "fwd_start")
            # NCHW -> NHWC in the compute type: nothing for a channels_last map that already has it, one launch for the others
            xs, recipes = {}, []
            need = [k for k in live if not _is_nhwc(feats[k], dt)]
            stack = torch.empty((sum(N * sizes[k][0] * sizes[k][1] for k in need), C), dtype=dt, device=dev) if need else None
            at = 0
            for k in live:
                h, w = sizes[k]
                f = feats[k].detach()
                if k not in need:
                    xs[k] = f.permute(0, 2, 3, 1)
                    continue
                if not f.is_contiguous():
                    f = f.contiguous()
                xs[k] = stack[at:at + N * h * w].view(N, h, w, C)
                at += N * h * w
                recipes.append(H.to_nhwc(f, xs[k]))
            H.permutes(recipes)
            H.mark(marks, "to_nhwc")
            Tm = torch.empty((M, C), dtype=dt, device=dev)
            wpack = head._pack("conv.weight", "c3", cw, dt)
            for i, k in enumerate(live):
                h, w = sizes[k]
                ops.gemm_nt(xs[k], wpack, cb.detach(), conv=1, act=L.ACT_RELU, out=Tm[first[i]:first[i] + N * h * w])
                H.mark(marks, f"conv_l{k}")
            lg, dl = predict(Tm, lsizes, N, wo.detach(), bo.detach(), wd.detach(), bd.detach())
            H.mark(marks, "predict")
            for i, k in enumerate(live):
                logits[k], deltas[k] = lg[i], dl[i]
        ctx.first = first
        ctx.save_for_backward(*[xs[k] for k in live], Tm, *params)
        if keep is not None:
            keep["x"], keep["T"], keep["first"] = [xs[k] for k in live], Tm.clone(), first       # the backward writes G over T
        return tuple(logits + deltas)

    @staticmethod
    def backward(ctx, *gouts):
        head, dt, keep, marks = ctx.cfg
        nl, N, sizes, live = ctx.nl, ctx.N, ctx.sizes, ctx.live
        C = head.in_channels
        need = ctx.needs_input_grad                              # (cfg, *features, *params)
        dev = gouts[0].device
        if not live:
            gf = [torch.zeros((N, C, h, w), dtype=ctx.f_dtypes[k], device=dev) if need[1 + k] else None for k, (h, w) in enumerate(sizes)]
            return (None,) + tuple(gf) + H.zeros_like_needed(ctx.saved_tensors, need[1 + nl:])
        H.once(ctx, "rpn_head", "hidden map")
        saved = ctx.saved_tensors
        xs, Tm, params = saved[:len(live)], saved[len(live)], saved[len(live) + 1:]
        cw, cb, wo, bo, wd, bd = params
        first = ctx.first
        lsizes = [sizes[k] for k in live]
        kept = {} if keep is not None else None
        grads = [None] * 6
        gfeat = [None] * nl
        with torch.cuda.device(dev):
            gmaps = [gouts[k] for k in live] + [gouts[nl + k] for k in live]
            gdt = dt if all(g.dtype == dt for g in gmaps) else torch.float32
            gmaps = [g.contiguous() if g.dtype == gdt else g.to(gdt).contiguous() for g in gmaps]
            if kept is not None:
                kept["dlogits"], kept["ddeltas"] = gmaps[:len(live)], gmaps[len(live):]
            H.mark(marks, "bwd_start")
            G, dwo, dbo, dwd, dbd = predict_bwd(Tm, lsizes, N, gmaps[:len(live)], gmaps[len(live):], wo.detach(), wd.detach())
            H.mark(marks, "predict_bwd")
            grads[2], grads[3], grads[4], grads[5] = dwo.view(wo.shape), dbo, dwd.view(wd.shape), dbd
            if need[1 + nl] or need[1 + nl + 1]:
                rows = [G[first[i]:first[i] + N * sizes[k][0] * sizes[k][1]] for i, k in enumerate(live)]    # one packed buffer for all levels
                grads[0], grads[1], dwk = H.conv3_param_grads(list(zip(rows, xs)), cw, cb, marks, [f"conv_wgrad_l{k}" for k in live])
                H.mark(marks, "conv_wgrad_unpack")
                if kept is not None:
                    kept["dwk"] = dwk
            if any(need[1 + k] for k in live):
                wdg = head._pack("conv.weight", "c3_d", cw, dt)
                recipes, dxs = [], []
                for i, k in enumerate(live):
                    if not need[1 + k]:
                        dxs.append(None)
                        continue
                    h, w = sizes[k]
                    dx = ops.gemm_nt(G[first[i]:first[i] + N * h * w].view(N, h, w, C), wdg, conv=1)
                    H.mark(marks, f"conv_dgrad_l{k}")
                    dxs.append(dx)
                    gfeat[k] = torch.empty((N, C, h, w), dtype=ctx.f_dtypes[k], device=dev)
                    recipes.append(H.to_nchw(dx, gfeat[k]))                                        # in the feature's type
                H.permutes(recipes)
                H.mark(marks, "to_nchw")
                if kept is not None:
                    kept["dx"] = dxs
            for k, (h, w) in enumerate(sizes):
                if k not in live and need[1 + k]:
                    gfeat[k] = torch.zeros((N, C, h, w), dtype=ctx.f_dtypes[k], device=dev)
            if kept is not None:
                kept["G"] = G
        if keep is not None:
            keep["grads"] = kept
        return (None,) + tuple(gfeat) + H.masked(grads, need[1 + nl:])


def _init(w):
    torch.nn.init.normal_(w, std=0.01)


class StandardRPNHead(torch.nn.Module):
    """Detectron2's StandardRPNHead with one hidden convolution: `conv` (3x3, C -> C, ReLU), `objectness_logits` (1x1, C -> A),
    `anchor_deltas` (1x1, C -> 4A).  The six parameters are float32 with Detectron2's names and shapes, so the
    `proposal_generator.rpn_head.*` entries of a checkpoint load with strict=True, and are initialised normal(std=0.01) with zero biases.

    forward(features): a list of [N, C, H_l, W_l] float32 or bfloat16 maps on the GPU (the same weights on every level) ->
    (pred_objectness_logits, pred_anchor_deltas): lists of [N, A, H_l, W_l] and [N, 4A, H_l, W_l] in the compute type (`compute_dtype`,
    else the first feature's), contiguous, as rpn.rpn_proposals and rpn_loss.rpn_losses read them.  One torch.autograd.Function over the
    features and the parameters; parameter gradients are float32 in the parameters' layouts, feature gradients in each feature's type.  A
    map that already is channels_last in the compute type is read in place.  The kernel-layout weight copies are cached and rebuilt when
    a parameter's version or the compute type changes.  Nothing is read back and nothing synchronises.  The backward overwrites the
    stored hidden map: it runs once per forward.  A level with N * H * W == 0 gives empty outputs that are still attached to the graph,
    and zero gradients.

    ValueError for argument errors before any launch, RuntimeError off the GPU."""

    def __init__(self, in_channels=256, num_anchors=3, box_dim=4, compute_dtype=None):
        super().__init__()
        if box_dim != 4:
            raise ValueError(f"rpn_head: only box dimension 4 is implemented, got box_dim={box_dim!r}")
        _check_shape(in_channels, num_anchors, "StandardRPNHead")
        H.check_compute_dtype(compute_dtype, "rpn_head")
        self.in_channels, self.num_anchors, self.box_dim, self.compute_dtype = in_channels, num_anchors, box_dim, compute_dtype
        self.conv = H.Layer((in_channels, in_channels, 3, 3), _init)
        self.objectness_logits = H.Layer((num_anchors, in_channels, 1, 1), _init)
        self.anchor_deltas = H.Layer((num_anchors * box_dim, in_channels, 1, 1), _init)
        self._cache = packs.PackCache()

    def _params(self):
        return [self.conv.weight, self.conv.bias, self.objectness_logits.weight, self.objectness_logits.bias, self.anchor_deltas.weight,
                self.anchor_deltas.bias]

    def _pack(self, name, kind, p, dt):
        return self._cache.get((name, kind, dt), p, lambda: packs.BUILDERS[kind](p, dt))

    def forward(self, features, *, _keep=None, _marks=None):
        if not isinstance(features, (list, tuple)) or not 1 <= len(features) <= MAX_LEVELS:
            raise ValueError(f"rpn_head: features is a list of between 1 and {MAX_LEVELS} [N, C, H, W] maps, got "
                             f"{type(features).__name__}{' of ' + str(len(features)) if isinstance(features, (list, tuple)) else ''}")
        M = 0
        for k, f in enumerate(features):
            if not isinstance(f, torch.Tensor) or f.dim() != 4 or f.dtype not in _DTYPES or f.shape[1] != self.in_channels:
                raise ValueError(f"rpn_head: features[{k}] must be float32 or bfloat16 [N, {self.in_channels}, H, W], got "
                                 f"{getattr(f, 'dtype', type(f))} {list(getattr(f, 'shape', []))}")
            if f.shape[0] != features[0].shape[0]:
                raise ValueError(f"rpn_head: features[{k}] has {int(f.shape[0])} images, features[0] has {int(features[0].shape[0])}")
            M += int(f.shape[0]) * int(f.shape[2]) * int(f.shape[3])
        if M >= 1 << 31:
            raise ValueError(f"rpn_head: {M} positions over all levels and images, 2^31 or more")
        params = self._params()
        H.check_master_copies(params, "rpn_head")
        T.one_device(list(features) + params, "rpn_head", "StandardRPNHead.forward")
        dt = self.compute_dtype or features[0].dtype
        out = _Head.apply((self, dt, _keep, _marks), *features, *params)
        nl = len(features)
        return list(out[:nl]), list(out[nl:])


class RPN(torch.nn.Module):
    """Detectron2's RPN (the proposal generator) on the device.  head: StandardRPNHead (registered as `rpn_head`, Detectron2's name);
    cells: rpn.cell_anchors' result; strides: the levels' strides.  pre_nms_topk / post_nms_topk: (training, inference) pairs.

    forward(images, features, gt_instances=None, *, seed=None, padded=False) -> (proposals, losses): images -- anything with
    `.image_sizes`, or the list of (h, w) itself; features -- a list, or a dict in level order; it runs the head; in training
    rpn_loss.label_and_sample_anchors (its sample is keyed by `seed`, a Python int per step, which training requires) and
    rpn_loss.rpn_losses on the ground truths' `gt_boxes` (items are dicts or objects) give {"loss_rpn_cls", "loss_rpn_loc"}, in eval mode
    losses is {}; in both modes rpn.rpn_proposals runs on the DETACHED outputs and `proposals` is exactly what it returns (padded=True:
    its padded form, no host read)."""

    def __init__(self, head, cells, strides, *, nms_thresh=0.7, pre_nms_topk=(2000, 1000), post_nms_topk=(1000, 1000), min_box_size=0.0,
                 batch_size_per_image=256, positive_fraction=0.5, iou_thresholds=(0.3, 0.7), anchor_boundary_thresh=-1,
                 box2box_weights=(1.0, 1.0, 1.0, 1.0), smooth_l1_beta=0.0, loss_weight=1.0, offset=0.0):
        super().__init__()
        if not isinstance(head, StandardRPNHead):
            raise ValueError(f"rpn_head: head must be a StandardRPNHead, got {type(head).__name__}")
        self.cells = rpn._check_cells(cells)
        self.strides, self.offset = rpn._check_strides(strides, len(self.cells), offset)
        if int(self.cells[0].shape[0]) != head.num_anchors:
            raise ValueError(f"rpn_head: the cells have {int(self.cells[0].shape[0])} anchors per position, the head {head.num_anchors}")
        for v, name in ((pre_nms_topk, "pre_nms_topk"), (post_nms_topk, "post_nms_topk")):
            if not isinstance(v, (list, tuple)) or len(v) != 2:
                raise ValueError(f"rpn_head: {name} is a (training, inference) pair, got {v!r}")
        self.rpn_head = head
        self.nms_thresh, self.pre_nms_topk, self.post_nms_topk, self.min_box_size = nms_thresh, tuple(pre_nms_topk), tuple(post_nms_topk), min_box_size
        self.batch_size_per_image, self.positive_fraction, self.iou_thresholds = batch_size_per_image, positive_fraction, tuple(iou_thresholds)
        self.anchor_boundary_thresh, self.box2box_weights, self.smooth_l1_beta = anchor_boundary_thresh, tuple(box2box_weights), smooth_l1_beta
        self.loss_weight = loss_weight

    def forward(self, images, features, gt_instances=None, *, seed=None, padded=False):
        image_sizes = list(getattr(images, "image_sizes", images))
        if isinstance(features, dict):
            feats = list(features.values())
        elif isinstance(features, (list, tuple)):
            feats = list(features)
        else:
            raise ValueError(f"rpn_head: features is a list or a dict of level maps in level order, got {type(features).__name__}")
        if len(feats) != len(self.cells):
            raise ValueError(f"rpn_head: {len(feats)} levels of features for {len(self.cells)} levels of anchors")
        gt_boxes = None
        if self.training:
            if seed is None:
                raise ValueError("rpn_head: training needs `seed`, the per-step key of the anchor sample (rpn_loss.label_and_sample_anchors)")
            if not isinstance(gt_instances, (list, tuple)) or len(gt_instances) != len(image_sizes):
                raise ValueError("rpn_head: training needs gt_instances, one item per image")
            gt_boxes = [T.unwrap(T.getter(item)("gt_boxes")) for item in gt_instances]
            if any(not isinstance(b, torch.Tensor) for b in gt_boxes):
                raise ValueError("rpn_head: every item of gt_instances needs gt_boxes")
        logits, deltas = self.rpn_head(feats)
        losses = {}
        k = 0 if self.training else 1
        if self.training:
            samples = rpn_loss.label_and_sample_anchors(
                self.cells, self.strides, [tuple(s.shape[2:]) for s in logits], gt_boxes, image_sizes, iou_thresholds=self.iou_thresholds,
                batch_size_per_image=self.batch_size_per_image, positive_fraction=self.positive_fraction,
                anchor_boundary_thresh=self.anchor_boundary_thresh, offset=self.offset, seed=seed)
            losses = rpn_loss.rpn_losses(logits, deltas, samples, self.cells, self.strides, gt_boxes, box2box_weights=self.box2box_weights,
                                         smooth_l1_beta=self.smooth_l1_beta, batch_size_per_image=self.batch_size_per_image,
                                         loss_weight=self.loss_weight, offset=self.offset)
        proposals = rpn.rpn_proposals([t.detach() for t in logits], [t.detach() for t in deltas], self.cells, self.strides, image_sizes,
                                      nms_thresh=self.nms_thresh, pre_nms_topk=self.pre_nms_topk[k], post_nms_topk=self.post_nms_topk[k],
                                      min_box_size=self.min_box_size, training=self.training, box2box_weights=self.box2box_weights,
                                      offset=self.offset, padded=padded)
        return proposals, losses
