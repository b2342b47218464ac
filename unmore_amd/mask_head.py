"""The mask head of the stage-3 detector on the device (cad/modeling/roi_heads/roi_heads.py:1098-1201, CustomMaskRCNNConvUpsampleHead,
and CustomStandardROIHeads._forward_mask :889-917): 3x3 convolutions with ReLU on the pooled [R,C,S,S] features, a 2x2 stride-2
ConvTranspose2d with ReLU, a 1x1 predictor -> [R,1,2S,2S] logits.  It sits between roi_pool.ROIPooler and mask_loss /
detector_inference.paste_masks.

The trunk is the library's implicit-GEMM convolution (ops.gemm_nt / gemm_tn with conv=1 on packs' weight layouts) and the
deconvolution one plain GEMM whose output D [R*S*S, 4C] keeps the (ky,kx,co) column order; the predictor, its gradient and the ReLU
mask of the deconvolution run straight on D (csrc/mask_head.hip: `tail_logits`, `tail_bwd`), so the [R,2S,2S,C] map is never laid
out.  Activations are stored in the compute type as the GEMMs round them and the tail kernels read those stored values: forward and
backward see the same ReLU masks.  No CPU fallback: tests/mask_head_common.py restates the head in float64 from torch's own ops."""
import torch

from . import _conv_head as H
from . import _lib as L
from . import _tables as T
from . import mask_loss, ops, packs, roi_sample
from .ops import _p, _stream

MAX_CHANNELS = H.MAX_CHANNELS
MAX_SIDE = 64
_DTYPES = H.DTYPES


def _check_tail(D, wp, bp, R, S, what):
    if not isinstance(D, torch.Tensor) or D.dtype not in _DTYPES or D.dim() != 2 or not D.is_contiguous():
        raise ValueError(f"mask_head: {what}: D must be contiguous float32 or bfloat16 [R*S*S, 4C], got {getattr(D, 'dtype', type(D))} "
                         f"{list(getattr(D, 'shape', []))}")
    if not isinstance(S, int) or isinstance(S, bool) or not 1 <= S <= MAX_SIDE:
        raise ValueError(f"mask_head: {what}: S must be an integer in [1, {MAX_SIDE}], got {S!r}")
    if not isinstance(R, int) or isinstance(R, bool) or R < 0 or R * S * S >= 1 << 31:
        raise ValueError(f"mask_head: {what}: R must be a non-negative integer with R*S*S < 2^31, got {R!r}")
    C = int(D.shape[1]) // 4
    if int(D.shape[0]) != R * S * S or D.shape[1] != 4 * C or C < 64 or C % 64 or C > MAX_CHANNELS:
        raise ValueError(f"mask_head: {what}: D must be [{R * S * S}, 4C] with C a multiple of 64 up to {MAX_CHANNELS}, got {list(D.shape)}")
    if not isinstance(wp, torch.Tensor) or wp.dtype != torch.float32 or wp.numel() != C or not wp.is_contiguous():
        raise ValueError(f"mask_head: {what}: wp must be contiguous float32 [{C}], got {getattr(wp, 'dtype', type(wp))} "
                         f"{list(getattr(wp, 'shape', []))}")
    if bp is not None and (not isinstance(bp, torch.Tensor) or bp.dtype != torch.float32 or bp.numel() != 1):
        raise ValueError(f"mask_head: {what}: bp must be float32 with one element, got {getattr(bp, 'dtype', type(bp))} "
                         f"{list(getattr(bp, 'shape', []))}")
    return C


def tail_logits(D, wp, bp, R, S, *, out_f32=False, sigmoid=False):
    """The predictor on the deconvolution GEMM's output (include/umr.h, umr_mask_head_logits): D [R*S*S, 4C] float32 or bfloat16,
    column (2*ky + kx)*C + co; wp float32 [C], bp float32 [1].  Returns [R,1,2S,2S] in D's type (float32 with out_f32):
    bp + sum_co D*wp at (2y + ky, 2x + kx), float32 sums; sigmoid=True stores the probability instead."""
    C = _check_tail(D, wp, bp, R, S, "tail_logits")
    dev = T.one_device([D, wp, bp], "mask_head", "tail_logits")
    with torch.cuda.device(dev):
        out = torch.empty((R, 1, 2 * S, 2 * S), dtype=torch.float32 if out_f32 else D.dtype, device=dev)
        L.check(L.lib().umr_mask_head_logits(_p(D), _p(wp), _p(bp), _p(out), R, S, C, T.dtype_code(D), int(bool(out_f32)), int(bool(sigmoid)),
                                             _stream()), "umr_mask_head_logits")
    return out


def tail_bwd(D, dlogits, wp, R, S, *, _phase_ms=None):
    """The predictor's backward and the deconvolution's ReLU mask in one pass over D (umr_mask_head_tail_bwd): D is OVERWRITTEN with
    G = (D > 0) * dlogit * wp[co], the float32 product rounded once to D's type.  dlogits: [R,1,2S,2S] in D's type or float32.
    Returns (G -- D itself --, dwp float32 [C], dbp float32 [1]); the two sums go through per-workgroup partials added in a fixed order,
    so the same input gives the same bytes."""
    C = _check_tail(D, wp, None, R, S, "tail_bwd")
    if not isinstance(dlogits, torch.Tensor) or dlogits.dtype not in (D.dtype, torch.float32) or dlogits.numel() != 4 * R * S * S \
            or not dlogits.is_contiguous():
        raise ValueError(f"mask_head: tail_bwd: dlogits must be contiguous [{R}, 1, {2 * S}, {2 * S}] in D's type or float32, got "
                         f"{getattr(dlogits, 'dtype', type(dlogits))} {list(getattr(dlogits, 'shape', []))}")
    dev = T.one_device([D, dlogits, wp], "mask_head", "tail_bwd")
    with torch.cuda.device(dev):
        dwp, dbp = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
        nbytes = L.lib().umr_mask_head_workspace(R * S * S, C)
        ws = T.workspace(nbytes, dev)

        def launch(phases):
            L.check(L.lib().umr_mask_head_tail_bwd(_p(D), _p(dlogits), int(dlogits.dtype == torch.float32), _p(wp), _p(dwp), _p(dbp), _p(ws),
                                                   nbytes, R, S, C, T.dtype_code(D), phases, _stream()), "umr_mask_head_tail_bwd")
        T.timed(launch, (("tail_bwd", 1), ("tail_finish", 2)), _phase_ms)
    return D, dwp, dbp


def _unpack_convT_grad(dwp, grad_out):  # [(i,j,co)][ci] f32 -> ConvTranspose2d's [ci,co,2,2] f32
    ci, co = grad_out.shape[0], grad_out.shape[1]
    return ops.permute4(dwp, grad_out, (ci, co, 2, 2), (1, ci, 2 * co * ci, co * ci))


class _Layers(torch.autograd.Function):
    """logits of (x, *parameters); cfg = (head, compute dtype, _keep, sigmoid, _marks)"""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        head, dt, keep, sigmoid, marks = cfg
        R, S = int(x.shape[0]), int(x.shape[2])
        ctx.cfg, ctx.R, ctx.S, ctx.x_dtype, ctx.done = cfg, R, S, x.dtype, False
        dev = x.device
        if R == 0:
            ctx.save_for_backward(*params)
            return torch.empty((0, 1, 2 * S, 2 * S), dtype=dt, device=dev)
        nconv = head.num_conv
        with torch.cuda.device(dev):
            cin = int(x.shape[1])
            a = torch.empty((R, S, S, cin), dtype=dt, device=dev)
            H.mark(marks, "fwd_start")
            H.permutes([H.to_nhwc(x.detach(), a)])                                               # cast to the compute type
            H.mark(marks, "to_nhwc")
            acts = [a]
            for k in range(nconv):
                w, b = params[2 * k], params[2 * k + 1]
                a = ops.gemm_nt(a, head._pack(f"mask_fcn{k + 1}.weight", "c3", w, dt), b.detach(), conv=1, act=L.ACT_RELU)
                a = a.view(R, S, S, -1)
                acts.append(a)
                H.mark(marks, f"mask_fcn{k + 1}")
            wd, bd, wpred, bpred = params[2 * nconv:2 * nconv + 4]
            brep = head._cache.get(("deconv.bias", "rep", torch.float32), bd, lambda: packs._rep_bias(bd, 4))
            D = ops.gemm_nt(a.view(R * S * S, -1), head._pack("deconv.weight", "ct", wd, dt), brep, act=L.ACT_RELU)
            H.mark(marks, "deconv")
            wp = wpred.detach().view(-1)
            logits = tail_logits(D, wp, bpred.detach(), R, S, sigmoid=sigmoid)
            H.mark(marks, "tail_logits")
        ctx.save_for_backward(*acts, D, *params)
        if keep is not None:
            keep["acts"], keep["D"] = acts, D.clone()          # the backward writes G over D
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        head, dt, keep, _, marks = ctx.cfg
        R, S = ctx.R, ctx.S
        nconv = head.num_conv
        need = ctx.needs_input_grad                              # (x, cfg, *params)
        if R == 0:
            gx = torch.zeros((0, head.in_channels, S, S), dtype=ctx.x_dtype, device=dlogits.device) if need[0] else None
            return (gx, None) + H.zeros_like_needed(ctx.saved_tensors, need[2:])
        H.once(ctx, "mask_head", "deconvolution output")
        saved = ctx.saved_tensors
        acts, D, params = saved[:nconv + 1], saved[nconv + 1], saved[nconv + 2:]
        wd, bd, wpred, bpred = params[2 * nconv:2 * nconv + 4]
        dev = D.device
        M = R * S * S
        grads = [None] * len(params)
        kept = {} if keep is not None else None
        with torch.cuda.device(dev):
            dl = dlogits.contiguous()
            if dl.dtype not in (dt, torch.float32):
                dl = dl.float()
            H.mark(marks, "bwd_start")
            G, dwp, dbp = tail_bwd(D, dl, wpred.detach().view(-1), R, S)
            H.mark(marks, "tail_bwd")
            grads[2 * nconv + 2], grads[2 * nconv + 3] = dwp.view(wpred.shape), dbp.view(bpred.shape)
            a4 = acts[nconv].view(M, -1)
            c4, c5 = int(wd.shape[0]), int(wd.shape[1])
            if need[2 + 2 * nconv] or need[2 + 2 * nconv + 1]:
                dbrep = torch.empty(4 * c5, dtype=torch.float32, device=dev)
                dwt = ops.gemm_tn(G, a4, dbias=dbrep)                                            # [(ky,kx,co)][ci]
                grads[2 * nconv] = _unpack_convT_grad(dwt, torch.empty_like(wd))
                grads[2 * nconv + 1] = ops.segsum(dbrep, 1, 4, c5, 0, c5).view(bd.shape)        # the four taps in tap order
                H.mark(marks, "deconv_wgrad")
            # the input of the deconvolution went through a ReLU unless it is x itself
            da = ops.gemm_nt(G, head._pack("deconv.weight", "ct_d", wd, dt), aux=(a4 if nconv else None), mask_relu=nconv > 0)
            H.mark(marks, "deconv_dgrad")
            if kept is not None:
                kept["G"], kept[f"da{nconv}"] = G, da
            for k in range(nconv, 0, -1):
                w, b = params[2 * (k - 1)], params[2 * (k - 1) + 1]
                below = acts[k - 1]
                if need[2 + 2 * (k - 1)] or need[2 + 2 * (k - 1) + 1]:
                    grads[2 * (k - 1)], grads[2 * (k - 1) + 1], _ = H.conv3_param_grads([(da.view(M, -1), below)], w, b)
                    H.mark(marks, f"mask_fcn{k}_wgrad")
                if k > 1:
                    da = ops.gemm_nt(da.view(R, S, S, -1), head._pack(f"mask_fcn{k}.weight", "c3_d", w, dt), conv=1, aux=below,
                                     mask_relu=True)
                elif need[0]:
                    da = ops.gemm_nt(da.view(R, S, S, -1), head._pack(f"mask_fcn{k}.weight", "c3_d", w, dt), conv=1)
                else:
                    da = None
                H.mark(marks, f"mask_fcn{k}_dgrad")
                if kept is not None:
                    kept[f"da{k - 1}"] = da
            gx = None
            if need[0]:
                gx = torch.empty((R, head.in_channels, S, S), dtype=ctx.x_dtype, device=dev)
                H.permutes([H.to_nchw(da, gx)])                                                  # in x's type
                H.mark(marks, "to_nchw")
        if keep is not None:
            keep["grads"] = kept
        return (gx, None) + H.masked(grads, need[2:])


def _msra_fill(w):                                               # c2_msra_fill
    torch.nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")


class MaskRCNNConvUpsampleHead(torch.nn.Module):
    """CustomMaskRCNNConvUpsampleHead for the class-agnostic recipe: len(conv_dims) - 1 3x3 convolutions with ReLU (`mask_fcn1` ...),
    `deconv` (ConvTranspose2d 2x2 stride 2) with ReLU, `predictor` (1x1, one class).  The parameters are float32 with the reference's
    names and shapes, so the `roi_heads.mask_head.*` entries of a Detectron2 checkpoint load with strict=True, and are initialised as
    the reference does (c2_msra_fill; normal(std=0.001) for the predictor; zero biases).

    layers(x): x [R, in_channels, S, S] float32 or bfloat16 on the GPU (what ROIPooler returns) -> logits [R,1,2S,2S] in the compute
    type (`compute_dtype`, else x's), one torch.autograd.Function over x and the parameters; parameter gradients are float32 in the
    parameters' own layouts.  The kernel-layout weight copies are cached and rebuilt when a parameter's version or the compute type
    changes.  Nothing is read back and nothing synchronises.  The backward overwrites the stored deconvolution output: it runs once
    per forward.  R == 0 gives empty logits that are still attached to the graph, and zero gradients.

    forward(x, instances): in training {"loss_mask": mask_loss.mask_rcnn_loss_weighted(logits, instances, weights=the instances'
    gt_scores) * loss_weight} (use_soft_targets) or the unweighted mask_rcnn_loss; in eval mode mask_rcnn_inference: the probabilities
    [R_i,1,2S,2S] of every image attached to its item as `pred_masks` (a dict's key, an object's attribute), split by the lengths of
    `pred_boxes`, and `instances` returned.  Items are dicts or objects with Detectron2's fields, as in mask_loss.

    ValueError for argument errors before any launch, RuntimeError off the GPU."""

    def __init__(self, in_channels=256, *, num_classes=1, conv_dims=(256,) * 5, use_soft_targets=True, loss_weight=1.0, vis_period=0,
                 compute_dtype=None, conv_norm=""):
        super().__init__()
        if num_classes != 1:
            raise ValueError(f"mask_head: only the class-agnostic head with one class is implemented, got num_classes={num_classes!r}")
        if conv_norm:
            raise ValueError(f"mask_head: normalised variants of the head are not implemented, got conv_norm={conv_norm!r}")
        conv_dims = tuple(conv_dims)
        if len(conv_dims) < 1:
            raise ValueError("mask_head: conv_dims have to be non-empty")
        for c in (in_channels,) + conv_dims:
            H.check_channels(c, "mask_head: every channel count")
        H.check_compute_dtype(compute_dtype, "mask_head")
        self.in_channels, self.conv_dims, self.num_conv = in_channels, conv_dims, len(conv_dims) - 1
        self.use_soft_targets, self.loss_weight, self.vis_period, self.compute_dtype = bool(use_soft_targets), loss_weight, vis_period, compute_dtype
        cur = in_channels
        for k, c in enumerate(conv_dims[:-1]):
            self.add_module(f"mask_fcn{k + 1}", H.Layer((c, cur, 3, 3), _msra_fill))
            cur = c
        self.deconv = H.Layer((cur, conv_dims[-1], 2, 2), _msra_fill, bias_dim=1)
        self.predictor = H.Layer((1, conv_dims[-1], 1, 1), lambda w: torch.nn.init.normal_(w, std=0.001))
        self._cache = packs.PackCache()

    def _params(self):
        ps = []
        for k in range(self.num_conv):
            m = getattr(self, f"mask_fcn{k + 1}")
            ps += [m.weight, m.bias]
        return ps + [self.deconv.weight, self.deconv.bias, self.predictor.weight, self.predictor.bias]

    def _pack(self, name, kind, p, dt):
        return self._cache.get((name, kind, dt), p, lambda: packs.BUILDERS[kind](p, dt))

    def layers(self, x, *, _keep=None, _sigmoid=False, _marks=None):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in _DTYPES or x.shape[1] != self.in_channels \
                or x.shape[2] != x.shape[3] or not 1 <= x.shape[2] <= MAX_SIDE:
            raise ValueError(f"mask_head: x must be float32 or bfloat16 [R, {self.in_channels}, S, S] with 1 <= S <= {MAX_SIDE}, got "
                             f"{getattr(x, 'dtype', type(x))} {list(getattr(x, 'shape', []))}")
        if x.shape[0] * x.shape[2] * x.shape[3] >= 1 << 31:
            raise ValueError("mask_head: R*S*S must be below 2^31")
        params = self._params()
        H.check_master_copies(params, "mask_head")
        T.one_device([x] + params, "mask_head", "MaskRCNNConvUpsampleHead.layers")
        if not x.is_contiguous():
            x = x.contiguous()
        dt = self.compute_dtype or x.dtype
        return _Layers.apply(x, (self, dt, _keep, _sigmoid, _marks), *params)

    def forward(self, x, instances):
        if self.training:
            logits = self.layers(x)
            if self.use_soft_targets:
                scores = [T.getter(item)("gt_scores") for item in instances]
                if any(not isinstance(s, torch.Tensor) for s in scores):
                    raise ValueError("mask_head: use_soft_targets needs gt_scores in every item of instances")
                weights = torch.cat(scores).detach() if scores else logits.new_zeros(0, dtype=torch.float32)
                loss = mask_loss.mask_rcnn_loss_weighted(logits, instances, weights=weights, vis_period=self.vis_period)
            else:
                loss = mask_loss.mask_rcnn_loss(logits, instances, vis_period=self.vis_period)
            return {"loss_mask": loss * self.loss_weight}
        lengths = []
        for k, item in enumerate(instances):
            boxes = T.unwrap(T.getter(item)("pred_boxes"))
            if not isinstance(boxes, torch.Tensor):
                raise ValueError(f"mask_head: instances[{k}] needs pred_boxes")
            lengths.append(int(boxes.shape[0]))
        if sum(lengths) != int(x.shape[0]):
            raise ValueError(f"mask_head: {int(x.shape[0])} rows of features for {sum(lengths)} pred_boxes")
        with torch.no_grad():
            probs = self.layers(x, _sigmoid=True)       # sigmoid of the float32 logit, rounded once: the logits kernel's own store
        for item, p in zip(instances, probs.split(lengths)):
            if isinstance(item, dict):
                item["pred_masks"] = p
            else:
                item.pred_masks = p
        return instances


def forward_mask(features, instances, pooler, head):
    """CustomStandardROIHeads._forward_mask: features -- the level maps the pooler takes, a list or a dict in level order; training:
    `instances` is roi_sample.label_and_sample_proposals' result, the head is trained on its foreground rows (roi_sample.foreground),
    pooled at their proposal_boxes; inference: the items' pred_boxes are pooled.  Returns what head(x, instances) returns."""
    feats = list(features.values()) if isinstance(features, dict) else list(features)
    if head.training:
        instances = roi_sample.foreground(instances)
        boxes = [T.unwrap(T.getter(item)("proposal_boxes")) for item in instances]
    else:
        boxes = [T.unwrap(T.getter(item)("pred_boxes")) for item in instances]
    if any(not isinstance(b, torch.Tensor) for b in boxes):
        raise ValueError("mask_head: forward_mask needs proposal_boxes (training) or pred_boxes (inference) in every item")
    return head(pooler(feats, boxes), instances)
