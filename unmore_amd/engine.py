"""Hand-scheduled forward / backward of the ObjectnessNet hot path on the HIP kernels.

This is the host-side "graph": an explicit list of kernel launches (no tracing
compiler, no autograd inside).  Activations are NHWC / [rows, channels]; weights
are repacked from the reference's PyTorch layouts into the layouts the kernels want
(cached per parameter version, packs.py).  Reference op order and formulas:
models/dpt/vit.py:165-201 (forward_flex), :86-90 (ProjectReadout), :104-145 +
:259-336 (reassemble), models/dpt/blocks.py:290-313 (RCU), :362-383 (fusion),
models/dpt/models.py:74-94 (DPT.forward), models/objectness_net.py:109-135,167-183
(heads), timm Block semantics as restated in SURVEY.md section 8c.

The list is written once.  Engine.forward picks a numerics object -- PlainNumerics here (bf16, and f32 on the exact-f32-MFMA
kernels) or engine_x3.X3Numerics (the fp32 parity mode on bf16 planes) -- and from there on names GEMMs, weight gradients and the
few steps the modes really do differently only through it; backward uses the numerics its forward saved.
"""
import os

import torch

from . import _lib as L
from . import graphs
from . import ops
from .engine_x3 import X3Numerics, _drop_f, _f
from .packs import (BUILDERS, ParamGroup, PackCache, _ACT, _pack_conv3, _pack_conv3_dgrad, _pack_convT, _pack_convT_dgrad, _pack_linear,
                    _pack_linear_t, _rep_bias, _unpack_conv3_grad)

CONFIGS = {
    # reference wiring: models/dpt/models.py:43-47, blocks.py:24-54, vit.py:515-543
    "dpt_large": dict(D=1024, depth=24, heads=16, patch=16, pos_grid=24, hooks=[5, 11, 17, 23], features=[256, 512, 1024, 1024]),
    "dpt_base": dict(D=768, depth=12, heads=12, patch=16, pos_grid=24, hooks=[2, 5, 8, 11], features=[96, 192, 384, 768]),
    # extensions named by BASELINE.json
    "dpt_small": dict(D=384, depth=12, heads=6, patch=16, pos_grid=24, hooks=[2, 5, 8, 11], features=[48, 96, 192, 384]),
    "dpt_large14": dict(D=1024, depth=24, heads=16, patch=14, pos_grid=37, hooks=[5, 11, 17, 23], features=[256, 512, 1024, 1024]),
    "dpt_tiny": dict(D=128, depth=4, heads=2, patch=16, pos_grid=24, hooks=[0, 1, 2, 3], features=[32, 64, 128, 128]),
}

_FUSE_HEAD_OUT = True   # the heads' 1024 -> {1,2} output layer in the epilogue of the GEMM before it (tests switch it off)
# A 1x1 convolution and a bilinear resize commute exactly (both linear, one per pixel across channels, the other per channel across
# pixels with weights that sum to 1, so the bias commutes too): conv1x1(resize(x)) == resize(conv1x1(x)).  The fusion blocks'
# out_conv (blocks.py:377-381: interpolate x2, then out_conv) and the first layer of both heads (objectness_net.py:110,121 on the
# x2-interpolated feature map, models.py:70-72) therefore run on the map BEFORE the resize -- a quarter of the rows in the GEMM, its
# weight gradient and its data gradient -- and the resize moves the GEMM's output.  False = the reference's order (tests).
_COMMUTE_RESIZE = True


_WGRAD_STREAM = os.environ.get("UMR_WGRAD_STREAM", "auto")   # weight gradients on a second stream: auto (small problems) | 0 | 1
_side_streams = {}


class WgradStream:
    """Weight gradients are leaves of the backward pass: nothing in it reads them.  For small problems (the reference's recipe:
    20 crops of 128x128, README.md:148-155 -- GEMMs of 24-264 tiles on 256 CUs) they run on a second HIP stream, beside the data-
    gradient chain instead of inside it; under a HIP-graph capture the fork and join are graph edges and cost the host nothing.
    Same kernels, same operands, same order per stream: results are bit-identical to the one-stream schedule.  Large problems
    fill the chip with every launch and keep one stream (and their memory: a tensor read on the side stream cannot be reused by
    the allocator until that stream has passed it)."""

    def __init__(self, dev, on):
        self.on = bool(on)
        # a staged capture in progress (graphs.StagedCaptured): the side-stream work is not launched here but deferred to the capture,
        # which records it as the stage's own graph at the next stage boundary and replays that graph on its second stream
        self.staged = graphs.staged() if self.on else None
        if self.on and self.staged is None:
            self.main = torch.cuda.current_stream(dev)
            key = (dev.index, self.main.cuda_stream)
            if key not in _side_streams:
                if len(_side_streams) > 16:
                    _side_streams.clear()
                _side_streams[key] = torch.cuda.Stream(device=dev)
            self.side = _side_streams[key]

    def run(self, fn, *used):
        """fn: launches on the current stream; used: tensors (allocated on the main stream) those launches read"""
        if not self.on:
            return fn()
        if self.staged is not None:
            return self.staged.defer(fn, used)
        self.side.wait_stream(self.main)       # the producers of `used` are enqueued on main
        graphs.note_fork(self.main, self.side)
        with torch.cuda.stream(self.side):
            fn()
        for t in used:
            if t is not None:
                t.record_stream(self.side)

    def stage_end(self):
        """a stage of backward is complete (engine.backward's cb): a staged capture closes the stage's graphs here"""
        if self.staged is not None:
            self.staged.boundary()

    def join(self):
        if self.on and self.staged is None:
            self.main.wait_stream(self.side)
        elif self.staged is not None:
            self.staged.join()

    @staticmethod
    def wanted(pixels):
        if _WGRAD_STREAM in ("0", "1"):
            return _WGRAD_STREAM == "1"
        return pixels <= graphs.AUTO_MAX_PIXELS


class PlainNumerics:
    """bf16 mode and the exact-f32-MFMA mode (UMR_F32_X3=0) behind Engine.forward / backward: a value is a plain tensor in the
    compute dtype and every GEMM is one ops.gemm_nt / gemm_tn launch.  Same interface as engine_x3.X3Numerics, one object per
    call: e = the Engine, P = its parameters."""

    def __init__(self, e, P):
        self.e, self.P = e, P

    def val(self, t):
        return t

    def to_dt(self, t):
        """an f32 tensor in the compute dtype"""
        return t if self.e.dt == torch.float32 else ops.cast(t, self.e.dt)

    def mm(self, A, wname, kind, bias=None, *, conv=0, act=L.ACT_NONE, want="f", mask=None, dgelu=None, aux=None, aux2=None,
           rowbias=None, rows_per_batch=0, c2_mode=0, c2_want="f", out=None, c_remap=None, aux_mod=0):
        """epi(A . W^T) with W = parameter `wname` in layout `kind` (Engine._w).  mask / dgelu / aux: the ONE [M, N] epilogue operand
        (keep where > 0 / times GELU'(.) / add).  want / c2_want (a format to ask for) mean nothing here."""
        a_t = mask if mask is not None else (dgelu if dgelu is not None else aux)
        return ops.gemm_nt(A, self.e._w(self.P, wname, kind), bias, out=out, aux=a_t, aux2=aux2, rowbias=rowbias,
                           rows_per_batch=rows_per_batch, act=act, mask_relu=mask is not None, mask_dgelu=dgelu is not None,
                           c2_mode=c2_mode, conv=conv, c_remap=c_remap, aux_mod=aux_mod)

    def wgrad(self, dY, X, dW, dbias=None, *, conv=0, wg=None, then=None):
        """dW = dY^T X (X NHWC with conv); with wg (a WgradStream) the launch and `then(dW)` go to the weight-gradient stream"""
        def launch():
            r = ops.gemm_tn(dY, X, dW=dW, dbias=dbias, conv=conv)
            if then is not None:
                then(r)
            return r
        return launch() if wg is None else wg.run(launch, dY, X)

    # ------------------------------------------------------------------ the steps of the schedule that are this mode's own
    def layernorm(self, x, gamma, beta):
        return ops.layernorm_fwd(x, gamma, beta)

    def readout(self, tok, wname, bias, save, B, g, Nt, D):
        """ProjectReadout (vit.py:86-90) on the hooked tokens [B*Nt, D]: the GEMM gathers the token rows itself, the class-token
        half of the weight [D, 2D] adds a per-image row bias; both halves are column slices of ONE pack"""
        P, dt = self.P, self.e.dt
        w_full = self.e.cache.get((wname, "lin", dt), P[wname], lambda: _pack_linear(P[wname], dt))  # [D, 2D]
        rb = ops.gemm_nt(tok, w_full[:, D:], bias, M=B, lda=Nt * D, out_f32=True)  # cls part + bias
        if save:
            r, rpre = ops.gemm_nt(tok, w_full[:, :D], None, rowbias=rb, rows_per_batch=g, act=L.ACT_GELU, c2_mode=2, M=B * g,
                                  a_remap=(g, Nt, 1))
        else:
            r, rpre = ops.gemm_nt(tok, w_full[:, :D], None, rowbias=rb, rows_per_batch=g, act=L.ACT_GELU, M=B * g,
                                  a_remap=(g, Nt, 1)), None
        return dict(r=r, rpre=rpre)

    def readout_wgrad(self, d_rpre, rs, tok, dW, B, g, Nt):
        """token half of the readout weight's gradient: the GEMM gathers the token rows"""
        ops.gemm_tn(d_rpre, tok, dW=dW, x_remap=(g, Nt, 1), M=B * g)

    def hook_grad(self, d_rpre, sB, wname, dx, B, g, Nt, D):
        """the readout's data gradient added into the token gradient dx [B*Nt, D] (created here at the last hook)"""
        dt = self.e.dt
        w = self.P[wname].detach()
        wa_t = self.e.cache.get((wname, "lin_t_a", dt), self.P[wname], lambda: _pack_linear_t(w[:, :D], dt))
        wb_t = self.e.cache.get((wname, "lin_t_b", dt), self.P[wname], lambda: _pack_linear_t(w[:, D:], dt))
        if dx is None:
            dx = torch.zeros((B * Nt, D), dtype=dt, device=sB.device)
        ops.gemm_nt(d_rpre, wa_t, None, out=dx, aux=dx, c_remap=(g, Nt, 1))
        cls_rows = dx.view(B, Nt * D)[:, :D]  # token 0 of every image: row stride Nt*D
        ops.gemm_nt(sB, wb_t, None, out=cls_rows, aux=cls_rows)
        return dx

    def head_resize(self, h1l, shape_low, H, W, relu):
        """resize(W1 path + b1), then the ReLU"""
        return ops.bilinear_fwd(h1l.view(*shape_low, -1), H, W, True, relu=relu).view(shape_low[0] * H * W, -1)

    def head_tail(self, h2, w3name, b3, w4, b4, act, final, keep, pre, B, H, W):
        """third and output layer of a factored head: (out, h3, pre-activation of the output or None)"""
        w3 = self.e._w(self.P, w3name, "lin")
        if _FUSE_HEAD_OUT and ops.gemm_nt(h2, w3, b3, act=act, query_rowreduce=True):
            # the 1024 -> {1,2} output layer rides in the epilogue of the GEMM that produces its input (one read of
            # h3 saved); without saved activations (inference) h3 is not written at all
            h3, parts = ops.gemm_nt(h2, w3, b3, act=act, red_w=w4.contiguous(), no_store=not keep)
            out = ops.head_out_finish(parts, b4, B, H, W, final)
            return out, h3, (ops.head_out_finish(parts, b4, B, H, W, L.ACT_NONE) if pre else None)
        h3 = ops.gemm_nt(h2, w3, b3, act=act)
        out = ops.head_out_fwd(h3, w4, b4, B, H, W, final)
        return out, h3, (ops.head_out_fwd(h3, w4, b4, B, H, W, L.ACT_NONE) if pre else None)

    def heads_backward(self, S, d_center, d_sdf, G, wgrad_lin, wgrad_c3, done):
        """Backward of both heads with their first layers' gradients side by side in one buffer (Engine._heads_backward_lowres /
        _fullres); done() closes the stage.  Returns the gradient of the map the last fusion block wrote."""
        e = self.e
        heads_bwd = e._heads_backward_lowres if S.get("path") is not None else e._heads_backward_fullres
        dpath = heads_bwd(self.P, S, d_center, d_sdf, G, wgrad_lin, wgrad_c3)
        done()
        return dpath

    def patch_wgrad(self, dx, patches, dW, dbias, B, g, Nt):
        """gradient of the patch-embedding weight (dW None: returned, in the padded layout of `patches`); the GEMM skips the
        class-token rows of dx"""
        return ops.gemm_tn(dx, patches, dW=dW, dbias=dbias, dy_remap=(g, Nt, 1), M=B * g)


class Engine:
    def __init__(self, cfg, head_layouts, compute_dtype=torch.float32, collapse_linear_heads=False, linear_head_backward=None):
        self.cfg = cfg
        # backward of a head without non-linearities between its convs (objectness_net.py:119-142): "algebraic" = exact gradients of
        # all eight factored tensors from three pixel reductions (no 512/1024-channel tensor is stored, read or multiplied in
        # backward); "gemm" = the layer-by-layer data/weight-gradient GEMMs (the round-1 form)
        self.linear_head_backward = linear_head_backward or "algebraic"
        assert self.linear_head_backward in ("algebraic", "gemm")
        self.center_layout, self.sdf_layout = head_layouts
        self.dt = compute_dtype
        self.cache = PackCache()
        # algebraic fast path for heads without non-linearities between their convs: "auto" (the net's
        # default) = such a head is evaluated as ONE 3x3 convolution at inference and, since round 6, in training whenever its
        # backward is the algebraic one (_collapse); True = always; False = never (the four convolutions as the reference runs them)
        assert collapse_linear_heads in (False, True, "auto")
        self.collapse_linear_heads = collapse_linear_heads

    # ------------------------------------------------------------------ collapsed linear head (opt-in)
    def _linear_head_weights(self, P, name, idx, dev):
        """The collapsed form of a linear head W4 W3 (W2 * (W1 x + b1) + b2) + b3) + b4 = one 3x3 conv 256 -> 1 plus a
        border-dependent bias.  All weight algebra is f32 on the master weights (element strides of the PyTorch layouts, no
        packing):  u = W4 W3 [512];  Vc[ci][t] = sum_co u[co] W2[co,ci,t];  Kw[t][c] = sum_ci Vc[ci][t] W1[ci][c];
        tb[t] = sum_ci Vc[ci][t] b1[ci] (t < 9);  tb[9] = u.b2 + W4.b3 + b4."""
        W1, b1 = self._f32(P, f"{name}.{idx[0]}.weight"), self._f32(P, f"{name}.{idx[0]}.bias")
        W2, b2 = self._f32(P, f"{name}.{idx[1]}.weight"), self._f32(P, f"{name}.{idx[1]}.bias")
        W3, b3 = self._f32(P, f"{name}.{idx[2]}.weight"), self._f32(P, f"{name}.{idx[2]}.bias")
        W4, b4 = self._f32(P, f"{name}.{idx[3]}.weight"), self._f32(P, f"{name}.{idx[3]}.bias")
        C, C1, C3 = W1.shape[1], W1.shape[0], W3.shape[0]  # 256, 512, 1024
        assert W4.shape[0] == 1 and W2.shape == (C1, C1, 3, 3) and all(t.is_contiguous() for t in (W1, W2, W3, W4))
        f = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        u, Vc, Kw, tb = f(C1), f(C1 * 9), f(9 * C), f(10)
        ops.small_gemm(W4, W3, u, 1, C1, C3, (0, 1), (C1, 1), (0, 1))
        ops.small_gemm(u, W2, Vc, 1, C1 * 9, C1, (0, 1), (C1 * 9, 1), (0, 1))
        ops.small_gemm(Vc, W1, Kw, 9, C, C1, (1, 9), (C, 1), (C, 1))
        ops.small_gemm(Vc, b1, tb, 9, 1, C1, (1, 9), (1, 0), (1, 0))
        ops.cast(b4, torch.float32, out=tb[9:10])
        ops.small_gemm(u, b2, tb[9:10], 1, 1, C1, (0, 1), (1, 0), (0, 0), accumulate=True)
        ops.small_gemm(W4, b3, tb[9:10], 1, 1, C3, (0, 1), (1, 0), (0, 0), accumulate=True)
        return u, Vc, Kw, tb

    def _collapse(self, lay, save):
        """does this call evaluate the head `lay` in its collapsed form?  (a head with ReLUs never; 'sine' is not invertible from
        its value, so its training step keeps the factored form whose backward gets the pre-activation)"""
        if lay["relu"] or (save and lay["final"] == "sine"):
            return False
        if self.collapse_linear_heads == "auto":
            # inference: always.  Training: when the head's backward is the algebraic one (the default) -- that backward reads the
            # head's OUTPUT only, so the 512 / 512 / 1024-channel maps of the four-convolution forward would be computed and thrown
            # away (qualified by tests/test_collapsed_train_gpu.py).  With the layer-by-layer GEMM
            # backward (set_linear_head_backward('gemm')) the forward keeps the four convolutions whose activations it reads.
            return (not save) or self.linear_head_backward == "algebraic"
        return bool(self.collapse_linear_heads)

    def _linear_head_weights_cached(self, P, name, idx, dev):
        """inference: the collapsed weights (and the 16-row tap matrix in the compute dtype) per version of the head's eight
        tensors (PackCache; dropped with the other non-replayable packs after an optimizer step of TrainStep)"""
        ps = [P[f"{name}.{i}.{t}"] for i in idx for t in ("weight", "bias")]

        def build():
            u, Vc, Kw, tb = self._linear_head_weights(P, name, idx, dev)
            return u, Vc, Kw, tb, self._tap_matrix(Kw)
        return self.cache.get((name, "collapsed", self.dt), ParamGroup(ps), build)

    def _tap_matrix(self, Kw):
        """[16, C] in the compute dtype: rows 0..8 = the nine tap vectors, the rest zero (the N = 16 operand of the tap GEMM)"""
        C = Kw.numel() // 9
        k16 = torch.zeros((16, C), dtype=torch.float32, device=Kw.device)
        k16[:9].copy_(Kw.view(9, C))
        return k16 if self.dt == torch.float32 else ops.cast(k16, self.dt)

    def _linear_head_forward_lowres(self, P, name, idx, path, H, W, act, save):
        """Collapsed forward of a head that reads the x2-interpolated feature map (models.py:70-72, objectness_net.py:128-135), taken
        BEFORE the resize: the nine tap products kw[t] . x are 1x1 products and commute with the resize (_COMMUTE_RESIZE), so they
        are one 16-column GEMM on the small map `path` [nb, ph, pw, 256]; the resize moves 16 f32 channels instead of 256, and
        lh_gather9_kernel sums every pixel's taps at their shifted positions (csrc/linear_head.hip).  The backward of a training
        step in this form is the algebraic one (it needs the output only)."""
        if save:
            u, Vc, Kw, tb = self._linear_head_weights(P, name, idx, path.device)
            k16 = self._tap_matrix(Kw)
        else:
            u, Vc, Kw, tb, k16 = self._linear_head_weights_cached(P, name, idx, path.device)
        nb, ph, pw, C = path.shape
        taps = ops.gemm_nt(path.reshape(-1, C), k16, None, out_f32=(self.dt != torch.float32))                    # [Ml, 16] f32
        taps = ops.bilinear_fwd(taps.view(nb, ph, pw, 16), H, W, True)                        # [B, H, W, 16] f32
        out = ops.linear_head_gather9(taps, tb, act)
        return out, dict(algebraic=True, act=act, out=out, u=u, Vc=Vc, Kw=Kw)

    def _linear_head_forward(self, P, name, idx, feat, act):
        """opt-in collapsed forward (csrc/linear_head.hip): the head as ONE streaming 3x3 conv 256 -> 1"""
        u, Vc, Kw, tb = self._linear_head_weights(P, name, idx, feat.device)
        out = ops.linear_head_fwd(feat, Kw, tb, act)
        return out, dict(collapsed=True, u=u, Vc=Vc, Kw=Kw, act=act)

    def _linear_head_backward(self, P, name, idx, feat, hs, dout, dfeat, G):
        """Gradients of every factored parameter from the three pixel reductions R = [G | n | D] (csrc/linear_head.hip)."""
        W1, b1 = self._f32(P, f"{name}.{idx[0]}.weight"), self._f32(P, f"{name}.{idx[0]}.bias")
        W2, b2 = self._f32(P, f"{name}.{idx[1]}.weight"), self._f32(P, f"{name}.{idx[1]}.bias")
        W3, b3 = self._f32(P, f"{name}.{idx[2]}.weight"), self._f32(P, f"{name}.{idx[2]}.bias")
        W4 = self._f32(P, f"{name}.{idx[3]}.weight")
        C, C1, C3 = W1.shape[1], W1.shape[0], W3.shape[0]
        dev = feat.device
        if "u" not in hs:   # factored forward, algebraic backward: the weight algebra is done here
            hs["u"], hs["Vc"], hs["Kw"], _ = self._linear_head_weights(P, name, idx, dev)
        act, u, Vc, Kw = hs["act"], hs["u"], hs["Vc"], hs["Kw"]
        dout = dout.contiguous()
        R = ops.linear_head_bwd_weight(feat, dout, hs["out"], act)
        Gm, n, D = R[:9 * C], R[9 * C:9 * C + 9], R[9 * C + 9:]
        # data gradient (accumulates into the centre head's dfeat when there is one)
        if dfeat is None:
            dfeat = torch.empty_like(feat)
            ops.linear_head_bwd_data(dout, hs["out"], Kw, dfeat, act, False)
        else:
            ops.linear_head_bwd_data(dout, hs["out"], Kw, dfeat.view(feat.shape), act, True)
        self._linear_head_algebra(P, name, idx, hs, Gm, n, D, G)
        return dfeat

    def _linear_head_algebra(self, P, name, idx, hs, Gm, n, D, G):
        """the factored parameters' gradients from G [9*C] (tap major), n [9], D [1] (all f32)"""
        W1, b1 = self._f32(P, f"{name}.{idx[0]}.weight"), self._f32(P, f"{name}.{idx[0]}.bias")
        W2, b2 = self._f32(P, f"{name}.{idx[1]}.weight"), self._f32(P, f"{name}.{idx[1]}.bias")
        W3, b3 = self._f32(P, f"{name}.{idx[2]}.weight"), self._f32(P, f"{name}.{idx[2]}.bias")
        W4 = self._f32(P, f"{name}.{idx[3]}.weight")
        C, C1, C3 = W1.shape[1], W1.shape[0], W3.shape[0]
        dev = Gm.device
        u, Vc = hs["u"], hs["Vc"]
        g = lambda k: (G[f"{name}.{idx[k]}.weight"], G[f"{name}.{idx[k]}.bias"])
        (gW1, gb1), (gW2, gb2), (gW3, gb3), (gW4, gb4) = g(0), g(1), g(2), g(3)
        gvc = torch.empty(C1 * 9, dtype=torch.float32, device=dev)
        gu = torch.empty(C1, dtype=torch.float32, device=dev)
        # gv[ci][t] = sum_c W1[ci][c] G[t][c] + n[t] b1[ci]
        ops.small_gemm(W1, Gm, gvc, C1, 9, C, (C, 1), (1, C), (9, 1))
        ops.small_gemm(b1, n, gvc, C1, 9, 1, (1, 0), (0, 1), (9, 1), accumulate=True)
        ops.small_gemm(Vc, Gm, gW1, C1, C, 9, (9, 1), (C, 1), (C, 1))           # dW1 = Vc G
        ops.small_gemm(Vc, n, gb1, C1, 1, 9, (9, 1), (1, 0), (1, 0))            # db1 = Vc n
        ops.small_gemm(u, gvc, gW2, C1, C1 * 9, 1, (1, 0), (0, 1), (C1 * 9, 1))  # dW2[co,ci,t] = u[co] gv[ci][t]
        ops.small_gemm(W2, gvc, gu, C1, 1, C1 * 9, (C1 * 9, 1), (1, 0), (1, 0))  # gu = W2 gv (+ D b2)
        ops.small_gemm(b2, D, gu, C1, 1, 1, (1, 0), (0, 0), (1, 0), accumulate=True)
        ops.small_gemm(u, D, gb2, C1, 1, 1, (1, 0), (0, 0), (1, 0))             # db2 = D u
        ops.small_gemm(gu, W3, gW4, 1, C3, C1, (0, 1), (1, C1), (0, 1))         # dW4 = gu W3^T (+ D b3)
        ops.small_gemm(D, b3, gW4, 1, C3, 1, (0, 0), (0, 1), (0, 1), accumulate=True)
        ops.small_gemm(W4, gu, gW3, C3, C1, 1, (1, 0), (0, 1), (C1, 1))         # dW3 = W4^T gu
        ops.small_gemm(W4, D, gb3, C3, 1, 1, (1, 0), (0, 0), (1, 0))            # db3 = D W4^T
        ops.cast(D, torch.float32, out=gb4.view(1))                              # db4 = D

    # ------------------------------------------------------------------ helpers
    def _w(self, P, name, kind):
        p = P[name]
        if kind == "lin" and self.dt == torch.float32 and p.dtype == torch.float32 and p.is_contiguous():
            return p.detach().reshape(p.shape[0], -1)    # fp32 mode: the [N, K] kernel layout IS the parameter's layout -- no copy
        return self.cache.get((name, kind, self.dt), p, lambda: BUILDERS[kind](p, self.dt))

    def _wx3(self, P, name, kind):
        """f32 weights as three bf16 planes per value ([rows, 3K]; conv: K = (ky,kx,ci) inside each plane) for ops.gemm_nt_x3.
        kinds: the layouts of _w plus 'lin_a' / 'lin_b' (/ 'lin_t_a' / 'lin_t_b'): the token / class-token column halves of the
        readout projection [D, 2D] (models/dpt/vit.py:84-88).  Refreshed after an optimizer step by the batched permute, straight
        from the parameter into the planes (PackCache.refresh)."""
        p = P[name]

        def pack_f32():
            w = p.detach()
            if kind == "lin":
                return w.reshape(w.shape[0], -1).contiguous()
            if kind in ("lin_a", "lin_b", "lin_t_a", "lin_t_b"):
                D = w.shape[1] // 2
                half = w[:, :D] if kind.endswith("a") else w[:, D:]
                if kind.startswith("lin_t"):
                    return _pack_linear_t(half, torch.float32)
                out = torch.empty((w.shape[0], D), dtype=torch.float32, device=w.device)
                return ops.permute4(w, out, (1, 1, w.shape[0], D), (0, 0, w.stride(0), 1), src_offset=(0 if kind.endswith("a") else D))
            return BUILDERS[kind](w, torch.float32)

        def build():
            return ops.split3(pack_f32())

        def recipe(rec, val):
            rowlen = val.shape[1] // 3
            if kind == "lin":          # no launch recorded: the pack is the parameter itself
                return (p.detach(), val, (1, 1, 1, p.numel()), (0, 0, 0, 1), 0, rowlen) if p.is_contiguous() else None
            return (rec[0][0], val, rec[0][2], rec[0][3], rec[0][4], rowlen) if len(rec) == 1 else None

        return self.cache.get((name, kind + "_x3"), p, build, recipe)

    def _f32(self, P, name):
        p = P[name].detach()
        assert p.dtype == torch.float32, "parameters must be fp32 (call .to(torch.float32))"
        return p

    # ------------------------------------------------------------------ forward
    def forward(self, P, images, save, skip=()):
        """P: dict name -> fp32 parameter tensor on the GPU (reference state-dict names).
        images: [B,3,H,W] fp32 on the GPU.  Returns (center [B,2,H,W] f32, sdf [B,1,H,W] f32, saved).
        skip (inference only): head module names that are not evaluated (their output is None) -- the boundary-reasoning rounds of
        object_reasoning.py:379-487 read the boundary-distance map alone, and the centre head is most of a 128x128 crop's forward."""
        cfg, dt = self.cfg, self.dt
        assert not (skip and save), "skip: inference only"
        # fp32 parity mode on the bf16-plane kernels (engine_x3.py), or plain tensors in the compute dtype: the launch list below
        # does not ask which
        nx = (X3Numerics if dt == torch.float32 and ops.get_f32_mode() in ("x3", "x3_fast") else PlainNumerics)(self, P)
        mm, val = nx.mm, nx.val
        b_ = lambda name: self._f32(P, name)
        assert images.is_cuda and images.dtype == torch.float32 and images.dim() == 4 and images.shape[1] == 3
        images = images.contiguous()
        B, _, H, W = images.shape
        p, D, heads = cfg["patch"], cfg["D"], cfg["heads"]
        gh, gw = H // p, W // p
        assert gh >= 1 and gw >= 1
        g, Nt = gh * gw, gh * gw + 1
        m = "backbone.pretrained.model."
        dev = images.device
        S = {"B": B, "H": H, "W": W, "gh": gh, "gw": gw, "numerics": type(nx)} if save else None

        # ---- patch embed + cls + pos (vit.py:168-193)
        G = cfg["pos_grid"]
        pos = b_(m + "pos_embed")[0]  # [1+G*G, D]
        if (gh, gw) != (G, G):
            pos_grid = ops.bilinear_fwd(pos[1:].reshape(1, G, G, D), gh, gw, False).reshape(g, D)
        else:
            pos_grid = pos[1:]
        pos_t = nx.to_dt(pos_grid.contiguous())
        K = 3 * p * p
        ldk = (K + 7) // 8 * 8
        patches = val(ops.patchify(images, p, dt, ldk))
        tokens = torch.empty((B * Nt, D), dtype=dt, device=dev)
        if ldk == K:
            mm(patches, m + "patch_embed.proj.weight", "lin", b_(m + "patch_embed.proj.bias"), out=tokens, aux=pos_t, aux_mod=g,
               c_remap=(g, Nt, 1))
        else:
            # rows padded to a multiple of 8 elements (patch 14): zero columns on the weight
            wp = self._w(P, m + "patch_embed.proj.weight", "lin")
            wpad = torch.zeros((D, ldk), dtype=dt, device=dev)
            wpad[:, :K] = wp
            ops.gemm_nt(_f(patches), wpad, b_(m + "patch_embed.proj.bias"), out=tokens, aux=pos_t, aux_mod=g, c_remap=(g, Nt, 1))
        ops.fill_cls(tokens, b_(m + "cls_token").reshape(-1), pos[0].contiguous(), B, Nt * D, D)
        if save:
            S["patches"] = patches

        # ---- transformer blocks (timm Block; only up to the last hooked block: later ones feed nothing, vit.py:107)
        # what only feeds GEMMs is asked for as want="p"; what LayerNorm, attention or a residual reads is taken as f32 (_f)
        x = tokens
        acts, blocks = [], []
        for i in range(max(cfg["hooks"]) + 1):
            b = m + f"blocks.{i}."
            ln1, mean1, rstd1 = nx.layernorm(x, b_(b + "norm1.weight"), b_(b + "norm1.bias"))
            qkv = _f(mm(ln1, b + "attn.qkv.weight", "lin", b_(b + "attn.qkv.bias")))
            att, lse = ops.attention_fwd(qkv, B, Nt, heads, need_lse=save)
            att = val(att)
            x1 = _f(mm(att, b + "attn.proj.weight", "lin", b_(b + "attn.proj.bias"), aux=x))
            ln2, mean2, rstd2 = nx.layernorm(x1, b_(b + "norm2.weight"), b_(b + "norm2.bias"))
            if save:
                h, hpre = mm(ln2, b + "mlp.fc1.weight", "lin", b_(b + "mlp.fc1.bias"), act=L.ACT_GELU, c2_mode=2, want="p")
            else:
                h, hpre = mm(ln2, b + "mlp.fc1.weight", "lin", b_(b + "mlp.fc1.bias"), act=L.ACT_GELU, want="p"), None
            x2 = _f(mm(h, b + "mlp.fc2.weight", "lin", b_(b + "mlp.fc2.bias"), aux=x1))
            if save:
                blocks.append(dict(x=x, mean1=mean1, rstd1=rstd1, ln1=ln1, qkv=qkv, att=att, lse=lse, x1=x1, mean2=mean2,
                                   rstd2=rstd2, ln2=ln2, hpre=hpre, h=h))
            x = x2
            if i in cfg["hooks"]:
                acts.append(x)
        if save:
            S["blocks"] = blocks
            S["acts"] = acts

        # ---- readout + reassemble (vit.py:86-90,104-145,259-336)
        pp = "backbone.pretrained."
        Fs = cfg["features"]
        layers, re_saved = [], []
        for k in range(4):
            a = pp + f"act_postprocess{k + 1}."
            rs = nx.readout(acts[k], a + "0.project.0.weight", b_(a + "0.project.0.bias"), save, B, g, Nt, D)
            F_ = Fs[k]
            # [B*g, F]; f32 where the stride-2 conv reads it
            f = mm(rs["r"], a + "3.weight", "lin", b_(a + "3.bias"), want=("f" if k == 3 else "p"))
            if k in (0, 1):
                s = 4 if k == 0 else 2
                bname = a + "4.bias"
                brep = self.cache.get((bname, "rep", s), P[bname], lambda: _rep_bias(P[bname], s * s))
                y = _f(mm(f, a + "4.weight", "ct", brep))
                lay = val(ops.pixel_shuffle(y, B, gh, gw, s, F_))
            elif k == 2:
                lay = f.view(B, gh, gw, F_)
            else:
                lay = mm(f.view(B, gh, gw, F_), a + "4.weight", "c3", b_(a + "4.bias"), conv=2)
                lay = lay.view(B, (gh - 1) // 2 + 1, (gw - 1) // 2 + 1, F_)
            layers.append(lay)
            if save:
                rs["f"] = f
                re_saved.append(rs)
        if save:
            S["re"] = re_saved

        # ---- scratch convs + refinenets (models.py:80-91, blocks.py:290-383)
        sc = "backbone.scratch."
        rn, rn_relu = [], []
        for k in range(4):
            lay = layers[k]
            o, orl = mm(lay, sc + f"layer{k + 1}_rn.weight", "c3", None, conv=1, c2_mode=1, c2_want="p")
            shp = (lay.shape[0], lay.shape[1], lay.shape[2], 256)
            rn.append(o.view(*shp))
            rn_relu.append(orl.view(*shp))
        fus_saved = {}
        path = None
        for k in (4, 3, 2, 1):
            r_ = sc + f"refinenet{k}."
            x1_, x1_relu = rn[k - 1], rn_relu[k - 1]
            nb, hh, ww, _ = x1_.shape
            shp = (nb, hh, ww, 256)
            fs = {}
            if path is None:
                s_, s_relu = x1_, x1_relu
            else:
                assert path.shape == x1_.shape, "fusion skip/size mismatch"
                t1 = mm(x1_relu, r_ + "resConfUnit1.conv1.weight", "c3", b_(r_ + "resConfUnit1.conv1.bias"), conv=1, act=L.ACT_RELU,
                        want="p").view(*shp)
                s_, s_relu = mm(t1, r_ + "resConfUnit1.conv2.weight", "c3", b_(r_ + "resConfUnit1.conv2.bias"), conv=1, aux=x1_, aux2=path,
                                c2_mode=1, c2_want="p")
                s_, s_relu = s_.view(*shp), s_relu.view(*shp)
                fs.update(x1_relu=x1_relu, t1=t1)
            t2 = mm(s_relu, r_ + "resConfUnit2.conv1.weight", "c3", b_(r_ + "resConfUnit2.conv1.bias"), conv=1, act=L.ACT_RELU,
                    want="p").view(*shp)
            u = mm(t2, r_ + "resConfUnit2.conv2.weight", "c3", b_(r_ + "resConfUnit2.conv2.bias"), conv=1, aux=s_).view(*shp)
            if k > 1 and cfg["patch"] != 16:
                nxt = rn[k - 2].shape
                Ho, Wo = nxt[1], nxt[2]  # patch-14 extension: resize to the next skip's size
            else:
                # the reference's wiring: exactly x2 (blocks.py:377-379); a token grid that does not survive the stride-2 conv and
                # the doublings (e.g. an odd grid) then fails at the skip addition, as the reference does (blocks.py:372)
                Ho, Wo = 2 * hh, 2 * ww
            if _COMMUTE_RESIZE:
                # out_conv before the resize (see _COMMUTE_RESIZE): its backward reads u, not the 4x larger resized map
                ul = mm(u.view(nb * hh * ww, 256), r_ + "out_conv.weight", "lin", b_(r_ + "out_conv.bias"))
                path = val(ops.bilinear_fwd(_f(ul).view(nb, hh, ww, 256), Ho, Wo, True))
                del ul
                src = ("u", u)
            else:
                up = val(ops.bilinear_fwd(_f(u), Ho, Wo, True))
                path = mm(up.view(nb * Ho * Wo, 256), r_ + "out_conv.weight", "lin", b_(r_ + "out_conv.bias")).view(nb, Ho, Wo, 256)
                src = ("up", up)
            if save:
                _drop_f(src[1])      # out_conv's weight gradient reads the planes, where there are any
                fs.update(s_relu=s_relu, t2=t2, in_hw=(hh, ww))
                fs[src[0]] = src[1]
                fus_saved[k] = fs
        if cfg["patch"] == 16:
            # models.py:70-72: Interpolate(scale_factor=2) -- the maps have 32 * (grid // 2 ...) = 16 * grid pixels per side, which is
            # the input size whenever that is a multiple of 16 (every documented use); otherwise smaller, exactly as in the reference
            H, W = 2 * path.shape[1], 2 * path.shape[2]
            if save:
                S["H"], S["W"] = H, W
        # the heads' first layer before the final resize (_COMMUTE_RESIZE): the interpolated 256-channel feature map is never
        # formed, and the backward of that layer -- weight gradient, data gradient, the algebraic head's reductions -- runs on
        # the quarter-size map
        lowres = _COMMUTE_RESIZE
        feat = val(ops.bilinear_fwd(_f(path), H, W, True)) if not lowres else None
        if save:
            S["fus"] = fus_saved
            S["rn_in"] = layers
            S["path1_hw"] = (path.shape[1], path.shape[2])
            S["feat"] = feat
            if lowres:
                S["path"] = path

        # ---- heads (objectness_net.py:109-135)
        outs, heads_saved = [], []
        M = B * H * W
        low = tuple(path.shape[:3])
        for name, lay in (("center_field_prediction_head", self.center_layout), ("sdf_prediction_head", self.sdf_layout)):
            if name in skip:
                outs.append(None)
                continue
            idx = lay["conv_idx"]
            final = _ACT[lay["final"]]
            if self._collapse(lay, save):
                if lowres:
                    out, cs = self._linear_head_forward_lowres(P, name, idx, _f(path), H, W, final, save)
                else:
                    out, cs = self._linear_head_forward(P, name, idx, _f(feat), final)
                    cs["out"] = out
                outs.append(out)
                if save:
                    heads_saved.append(cs)
                continue
            act = L.ACT_RELU if lay["relu"] else L.ACT_NONE
            # a head that is linear up to its output activation needs none of its 512/1024-channel activations in backward
            # (exact gradients from three pixel reductions over feat, _linear_head_backward); sin is not invertible from its value
            algebraic = save and not lay["relu"] and lay["final"] != "sine" and self.linear_head_backward == "algebraic"
            keep = save and not algebraic
            hw, hb = (lambda j: f"{name}.{idx[j]}.weight"), (lambda j: b_(f"{name}.{idx[j]}.bias"))
            if lowres:
                h1l = mm(path.view(low[0] * low[1] * low[2], 256), hw(0), "lin", hb(0))
                h1 = nx.head_resize(h1l, low, H, W, lay["relu"])
                del h1l
            else:
                h1 = mm(feat.view(M, 256), hw(0), "lin", hb(0), act=act, want="p")
            h2 = mm(h1.view(B, H, W, 512), hw(1), "c3", hb(1), conv=1, act=act, want="p")
            w4 = b_(hw(3))
            # sin is not invertible from its value: the backward pass of the 'sine' variant gets the pre-activation
            out, h3, zpre = nx.head_tail(h2, hw(2), hb(2), w4.reshape(w4.shape[0], -1), hb(3), act, final, keep,
                                         save and lay["final"] == "sine", B, H, W)
            outs.append(out)
            if algebraic:
                heads_saved.append(dict(algebraic=True, act=final, out=out))
            elif save:
                heads_saved.append(dict(h1=h1, h2=h2, h3=h3, out=(zpre if zpre is not None else out)))
            del h1, h2, h3
        if save:
            S["heads"] = heads_saved
        return outs[0], outs[1], S

    def _heads_backward_fullres(self, P, S, d_center, d_sdf, G, wgrad_lin, wgrad_c3):
        """backward of both heads on the interpolated feature map (the reference's order of operations); returns the gradient of the
        map before the final resize"""
        dt = self.dt
        B, H, W = S["B"], S["H"], S["W"]
        dev = d_center.device
        dfeat = None
        feat = S["feat"]
        # Both heads factored: their layer-1 input gradients dh1 go side by side into one [M, 2*C1] buffer and the gradient of
        # the shared feature map is ONE GEMM over K = 2*C1 (instead of a GEMM plus a second one that re-reads and re-writes
        # the [M, 256] result to accumulate into it).
        merge_dfeat = all(not (hs_.get("collapsed") or hs_.get("algebraic")) for hs_ in S["heads"])
        dh1cat, w1cat = None, []
        for hi, (name, lay, dout) in enumerate((("center_field_prediction_head", self.center_layout, d_center),
                                               ("sdf_prediction_head", self.sdf_layout, d_sdf))):
            hs = S["heads"][hi]
            idx = lay["conv_idx"]
            if hs.get("collapsed") or hs.get("algebraic"):
                dfeat = self._linear_head_backward(P, name, idx, feat, hs, dout, dfeat, G)
                continue
            relu = lay["relu"]
            w4 = self._f32(P, f"{name}.{idx[3]}.weight")
            dh3 = ops.head_out_bwd(hs["h3"], w4.reshape(w4.shape[0], -1), dout.contiguous(), hs["out"], _ACT[lay["final"]], relu,
                                   G[f"{name}.{idx[3]}.weight"].view(w4.shape[0], -1), G[f"{name}.{idx[3]}.bias"])
            hs["h3"] = None
            wgrad_lin(f"{name}.{idx[2]}.weight", dh3, hs["h2"], f"{name}.{idx[2]}.bias")
            dh2 = ops.gemm_nt(dh3, self._w(P, f"{name}.{idx[2]}.weight", "lin_t"), None, aux=(hs["h2"] if relu else None), mask_relu=relu)
            del dh3
            h1 = hs["h1"].view(B, H, W, 512)
            wgrad_c3(f"{name}.{idx[1]}.weight", dh2, h1, f"{name}.{idx[1]}.bias")
            hs["h2"] = None
            c1 = hs["h1"].shape[-1]
            if merge_dfeat and dh1cat is None:
                dh1cat = torch.empty((B * H * W, 2 * c1), dtype=dt, device=dev)
            dh1 = ops.gemm_nt(dh2.view(B, H, W, 512), self._w(P, f"{name}.{idx[1]}.weight", "c3_d"), None, conv=1,
                              aux=(hs["h1"] if relu else None), mask_relu=relu,
                              out=(dh1cat[:, hi * c1:(hi + 1) * c1] if merge_dfeat else None))
            del dh2
            hs["h1"] = None
            wgrad_lin(f"{name}.{idx[0]}.weight", dh1, feat.view(-1, 256), f"{name}.{idx[0]}.bias")
            if merge_dfeat:
                w1cat.append(self._w(P, f"{name}.{idx[0]}.weight", "lin_t"))
            elif dfeat is None:
                dfeat = ops.gemm_nt(dh1, self._w(P, f"{name}.{idx[0]}.weight", "lin_t"), None)
            else:
                ops.gemm_nt(dh1, self._w(P, f"{name}.{idx[0]}.weight", "lin_t"), None, aux=dfeat, out=dfeat)
            del dh1
        if merge_dfeat:
            dfeat = ops.gemm_nt(dh1cat, torch.cat(w1cat, dim=1), None)
            del dh1cat
        S["feat"] = None
        ph, pw = S["path1_hw"]
        dpath = ops.bilinear_bwd(dfeat.view(B, H, W, 256), ph, pw, True)
        del dfeat
        return dpath

    def _heads_backward_lowres(self, P, S, d_center, d_sdf, G, wgrad_lin, wgrad_c3):
        """Backward of both heads when their first layer ran before the final resize (_COMMUTE_RESIZE).  The gradient of that layer's
        OUTPUT goes through the resize's adjoint -- the 512 channels of a factored head, the 16-channel map of shifted output
        gradients of an algebraic head (csrc/linear_head.hip, lh_shift9_kernel) -- side by side into ONE [Ml, K] buffer on the small
        map; the layer's weight gradients, the algebraic head's tap reductions and the gradient of the small map (one GEMM over K)
        are taken there.  Returns that gradient [nb, ph, pw, 256]."""
        dt = self.dt
        B, H, W = S["B"], S["H"], S["W"]
        path = S["path"]
        nb, ph, pw, C = path.shape
        pl = path.view(-1, C)
        Ml = pl.shape[0]
        dev = path.device
        widths = [64 if hs_.get("algebraic") else hs_["h1"].shape[-1] for hs_ in S["heads"]]
        K = sum(widths)
        dlow = torch.empty((Ml, K), dtype=dt, device=dev)
        bcat = torch.zeros((C, K), dtype=dt, device=dev)          # [256, K]: dpath = dlow . bcat^T
        c0 = 0
        for hi, (name, lay, dout) in enumerate((("center_field_prediction_head", self.center_layout, d_center),
                                               ("sdf_prediction_head", self.sdf_layout, d_sdf))):
            hs = S["heads"][hi]
            idx = lay["conv_idx"]
            if hs.get("algebraic"):     # (also a head whose FORWARD ran collapsed: _linear_head_forward_lowres)
                if "u" not in hs:
                    hs["u"], hs["Vc"], hs["Kw"], _ = self._linear_head_weights(P, name, idx, dev)
                s9, nd = ops.linear_head_shift9(dout.contiguous(), hs["out"], hs["act"], dt)
                ops.bilinear_bwd(s9, ph, pw, True, out=dlow[:, c0:c0 + 16].unflatten(0, (nb, ph, pw)))
                del s9
                dlow[:, c0 + 16:c0 + 64].zero_()
                gm = ops.gemm_tn(dlow[:, c0:c0 + 16], pl)           # [16, 256]: G[t][c] = sum_q (U^T s9)[q][t] path(q)[c]
                self._linear_head_algebra(P, name, idx, hs, gm[:9].reshape(-1), nd[:9], nd[9:10], G)
                bcat[:, c0:c0 + 9].copy_(hs["Kw"].view(9, C).t())
                c0 += 64
                continue
            relu = lay["relu"]
            w4 = self._f32(P, f"{name}.{idx[3]}.weight")
            dh3 = ops.head_out_bwd(hs["h3"], w4.reshape(w4.shape[0], -1), dout.contiguous(), hs["out"], _ACT[lay["final"]], relu,
                                   G[f"{name}.{idx[3]}.weight"].view(w4.shape[0], -1), G[f"{name}.{idx[3]}.bias"])
            hs["h3"] = None
            wgrad_lin(f"{name}.{idx[2]}.weight", dh3, hs["h2"], f"{name}.{idx[2]}.bias")
            dh2 = ops.gemm_nt(dh3, self._w(P, f"{name}.{idx[2]}.weight", "lin_t"), None, aux=(hs["h2"] if relu else None), mask_relu=relu)
            del dh3
            c1 = hs["h1"].shape[-1]
            wgrad_c3(f"{name}.{idx[1]}.weight", dh2, hs["h1"].view(B, H, W, c1), f"{name}.{idx[1]}.bias")
            hs["h2"] = None
            dh1 = ops.gemm_nt(dh2.view(B, H, W, -1), self._w(P, f"{name}.{idx[1]}.weight", "c3_d"), None, conv=1,
                              aux=(hs["h1"] if relu else None), mask_relu=relu)
            del dh2
            hs["h1"] = None
            ops.bilinear_bwd(dh1.view(B, H, W, c1), ph, pw, True, out=dlow[:, c0:c0 + c1].unflatten(0, (nb, ph, pw)))
            del dh1
            wgrad_lin(f"{name}.{idx[0]}.weight", dlow[:, c0:c0 + c1], pl, f"{name}.{idx[0]}.bias")
            bcat[:, c0:c0 + c1].copy_(self._w(P, f"{name}.{idx[0]}.weight", "lin_t"))
            c0 += c1
        dpath = ops.gemm_nt(dlow, bcat, None).view(nb, ph, pw, C)
        S["path"] = None
        S["feat"] = None
        return dpath

    # ------------------------------------------------------------------ backward
    def backward(self, P, S, d_center, d_sdf, G, stage_cb=None, join_at_stages=False):
        """G: dict name -> preallocated fp32 gradient tensor (parameter shape) to fill.
        Parameters that receive no gradient are left untouched.
        stage_cb(name, wg) is called when a stage's gradients are complete or enqueued behind wg (the WgradStream of this pass):
        the data-parallel exchange launches its bucket there, a single-GPU step enqueues the stage's Adam update behind wg;
        join_at_stages: the caller reads the gradients inside stage_cb (so the weight-gradient stream is joined before each call)."""
        cfg = self.cfg
        nx = S["numerics"](self, P)       # the numerics of the forward that saved S
        mm, val = nx.mm, nx.val
        B, H, W, gh, gw = S["B"], S["H"], S["W"], S["gh"], S["gw"]
        D, heads, p = cfg["D"], cfg["heads"], cfg["patch"]
        g, Nt = gh * gw, gh * gw + 1
        dev = d_center.device
        wg = WgradStream(dev, WgradStream.wanted(B * H * W))
        # LayerNorm's dgamma / dbeta are weight gradients too: in a chain-of-graphs step their reduction pass leaves the data-gradient chain
        # for the weight-gradient lane (48 launches of the reference recipe's step; +0.7 %).  Not in the eager two-stream schedule, whose
        # host is the slower side in backward: a hand-over costs it more than the 4-us kernel costs the GPU.
        ln_via = wg.run if wg.staged is not None else None

        def cb(name):
            if join_at_stages:
                wg.join()
            if stage_cb is not None:
                stage_cb(name, wg)
            wg.stage_end()

        def wgrad_lin(name, dy, x, bias_name=None):
            nx.wgrad(dy, x, G[name].view(G[name].shape[0], -1), (G[bias_name] if bias_name else None), wg=wg)

        def wgrad_c3(name, dy, x_nhwc, bias_name=None, conv=1):
            co = G[name].shape[0]
            nx.wgrad(dy.view(-1, co), x_nhwc, None, (G[bias_name] if bias_name else None), conv=conv, wg=wg,
                     then=lambda dwp: _unpack_conv3_grad(dwp, G[name]))

        # ---- heads: the gradient of the last fusion block's output
        dpath = nx.heads_backward(S, d_center, d_sdf, G, wgrad_lin, wgrad_c3, lambda: cb("heads"))

        # ---- refinenets + scratch convs
        sc = "backbone.scratch."
        d_rn = {}
        for k in (1, 2, 3, 4):
            r_ = sc + f"refinenet{k}."
            fs = S["fus"][k]
            hh, ww = fs["in_hw"]
            nb, Hp, Wp = dpath.shape[0], dpath.shape[1], dpath.shape[2]
            shp = (nb, hh, ww, 256)
            if "u" in fs:    # out_conv ran before the resize (_COMMUTE_RESIZE)
                dul = val(ops.bilinear_bwd(_f(dpath), hh, ww, True)).view(nb * hh * ww, 256)
                wgrad_lin(r_ + "out_conv.weight", dul, fs["u"].view(nb * hh * ww, 256), r_ + "out_conv.bias")
                du = mm(dul, r_ + "out_conv.weight", "lin_t", None).view(*shp)
                del dul
            else:
                dp2 = dpath.view(nb * Hp * Wp, 256)
                wgrad_lin(r_ + "out_conv.weight", dp2, fs["up"].view(nb * Hp * Wp, 256), r_ + "out_conv.bias")
                dup = _f(mm(dp2, r_ + "out_conv.weight", "lin_t", None))
                du = val(ops.bilinear_bwd(dup.view(nb, Hp, Wp, 256), hh, ww, True))
                del dup
            # RCU2: u = conv2(relu(conv1(relu(s)))) + s
            wgrad_c3(r_ + "resConfUnit2.conv2.weight", du, fs["t2"], r_ + "resConfUnit2.conv2.bias")
            dt2 = mm(du, r_ + "resConfUnit2.conv2.weight", "c3_d", None, conv=1, mask=fs["t2"], want="p").view(*shp)
            wgrad_c3(r_ + "resConfUnit2.conv1.weight", dt2, fs["s_relu"], r_ + "resConfUnit2.conv1.bias")
            ds = mm(dt2, r_ + "resConfUnit2.conv1.weight", "c3_d", None, conv=1, mask=fs["s_relu"], aux2=du, want="p").view(*shp)
            del dt2, du
            if "t1" in fs:
                # s = path_prev + RCU1(x1)
                wgrad_c3(r_ + "resConfUnit1.conv2.weight", ds, fs["t1"], r_ + "resConfUnit1.conv2.bias")
                dt1 = mm(ds, r_ + "resConfUnit1.conv2.weight", "c3_d", None, conv=1, mask=fs["t1"], want="p").view(*shp)
                wgrad_c3(r_ + "resConfUnit1.conv1.weight", dt1, fs["x1_relu"], r_ + "resConfUnit1.conv1.bias")
                dx1 = mm(dt1, r_ + "resConfUnit1.conv1.weight", "c3_d", None, conv=1, mask=fs["x1_relu"], aux2=ds, want="p").view(*shp)
                del dt1
                d_rn[k] = dx1
                dpath = ds  # gradient of the previous (coarser) path
            else:
                d_rn[k] = ds
            S["fus"][k] = None

        cb("refine")
        # ---- layerK_rn + reassemble + readout; token gradients collected per hook
        pp = "backbone.pretrained."
        Fs = cfg["features"]
        d_hook = [None] * 4  # (d_rpre [B*g, D], sB [B, D], readout weight's name) applied to the token gradient when the block is reached
        for k in range(4):
            lay_in = S["rn_in"][k]
            dr = d_rn.pop(k + 1)
            wgrad_c3(sc + f"layer{k + 1}_rn.weight", dr, lay_in, None)
            # dl: gradient of the reassembled map; f32 where a non-GEMM kernel (pixel shuffle, zero stuffing) or the stride-2
            # weight gradient reads it
            dl = mm(dr, sc + f"layer{k + 1}_rn.weight", "c3_d", None, conv=1, want=("p" if k == 2 else "f"))
            del dr
            a = pp + f"act_postprocess{k + 1}."
            F_ = Fs[k]
            rs = S["re"][k]
            f = rs["f"]
            if k in (0, 1):
                s = 4 if k == 0 else 2
                dyu = val(ops.pixel_shuffle(_f(dl).view(B, gh * s, gw * s, F_), B, gh, gw, s, F_, inverse=True))  # [B*g, s*s*F]
                brep = torch.empty(s * s * F_, dtype=torch.float32, device=dev)
                dwp = nx.wgrad(dyu, f.view(B * g, F_), None, brep)  # [(i,j,co)][ci]
                gw_ = G[a + "4.weight"]  # [ci, co, s, s]
                ops.permute4(dwp, gw_, (F_, F_, s, s), (1, F_, s * F_ * F_, F_ * F_))
                ops.segsum(brep, 1, s * s, F_, 0, F_, out=G[a + "4.bias"].view(1, F_))
                df = mm(dyu, a + "4.weight", "ct_d", None, want="p")
                del dyu
            elif k == 2:
                df = dl.view(B * g, F_)
            else:
                ho, wo = (gh - 1) // 2 + 1, (gw - 1) // 2 + 1
                wgrad_c3(a + "4.weight", dl, f.view(B, gh, gw, F_), a + "4.bias", conv=2)
                stuffed = val(ops.zero_stuff2(_f(dl).view(B, ho, wo, F_), gh, gw))
                df = mm(stuffed, a + "4.weight", "c3_d", None, conv=1, want="p").view(B * g, F_)
                del stuffed
            del dl
            wgrad_lin(a + "3.weight", df, rs["r"], a + "3.bias")
            d_rpre = mm(df, a + "3.weight", "lin_t", None, dgelu=rs["rpre"], want="p")  # [B*g, D]
            del df
            tok = S["acts"][k]
            wname = a + "0.project.0.weight"
            gfull = G[wname]  # [D, 2D]: token half | class-token half
            nx.readout_wgrad(d_rpre, rs, tok, gfull[:, :D], B, g, Nt)
            sB32 = ops.segsum(_f(d_rpre), B, g, D, g * D, D)  # [B, D] f32: sum over patches
            ops.segsum(sB32, 1, B, D, 0, D, out=G[a + "0.project.0.bias"].view(1, D))
            sB = nx.to_dt(sB32)
            ops.gemm_tn(sB, tok, dW=gfull[:, D:], M=B, ldx=Nt * D)   # class-token half: B rows (tiny)
            d_hook[k] = (d_rpre, sB, wname)
            S["re"][k] = None

        cb("reassemble")

        # ---- transformer blocks
        m = "backbone.pretrained.model."
        dx = None
        hooks = cfg["hooks"]
        for i in range(max(hooks), -1, -1):
            if i in hooks:
                k = hooks.index(i)
                dx = nx.hook_grad(*d_hook[k], dx, B, g, Nt, D)
                d_hook[k] = None
            b = m + f"blocks.{i}."
            bs = S["blocks"][i]
            dxx = val(dx)
            wgrad_lin(b + "mlp.fc2.weight", dxx, bs["h"], b + "mlp.fc2.bias")
            dhp = mm(dxx, b + "mlp.fc2.weight", "lin_t", None, dgelu=bs["hpre"], want="p")
            wgrad_lin(b + "mlp.fc1.weight", dhp, bs["ln2"], b + "mlp.fc1.bias")
            dln2 = _f(mm(dhp, b + "mlp.fc1.weight", "lin_t", None))
            del dhp, dxx
            dx1 = ops.layernorm_bwd(dln2, bs["x1"], self._f32(P, b + "norm2.weight"), bs["mean2"], bs["rstd2"],
                                    G[b + "norm2.weight"], G[b + "norm2.bias"], dres=dx, params_via=ln_via)
            del dln2
            dx1x = val(dx1)
            wgrad_lin(b + "attn.proj.weight", dx1x, bs["att"], b + "attn.proj.bias")
            datt = _f(mm(dx1x, b + "attn.proj.weight", "lin_t", None))
            dqkv = val(ops.attention_bwd(bs["qkv"], _f(bs["att"]), datt, bs["lse"], B, Nt, heads))
            del datt, dx1x
            wgrad_lin(b + "attn.qkv.weight", dqkv, bs["ln1"], b + "attn.qkv.bias")
            dln1 = _f(mm(dqkv, b + "attn.qkv.weight", "lin_t", None))
            del dqkv
            dx = ops.layernorm_bwd(dln1, bs["x"], self._f32(P, b + "norm1.weight"), bs["mean1"], bs["rstd1"],
                                   G[b + "norm1.weight"], G[b + "norm1.bias"], dres=dx1, params_via=ln_via)
            del dln1, dx1
            S["blocks"][i] = None
            cb(f"block{i}")

        # ---- embeddings (vit.py:179-193)
        dpos = ops.segsum(dx, Nt, B, Nt * D, D, D)  # [Nt, D] f32, sum over images
        G[m + "cls_token"].view(-1).copy_(dpos[0])
        gpos = G[m + "pos_embed"]
        Gd = cfg["pos_grid"]
        gpos[0, 0].copy_(dpos[0])
        if (gh, gw) == (Gd, Gd):
            gpos[0, 1:].copy_(dpos[1:])
        else:
            gpos[0, 1:].copy_(ops.bilinear_bwd(dpos[1:].reshape(1, gh, gw, D).contiguous(), Gd, Gd, False).view(Gd * Gd, D))
        K = 3 * p * p
        gwp = G[m + "patch_embed.proj.weight"].view(D, K)
        patches = S["patches"]
        if patches.shape[1] == K:
            nx.patch_wgrad(dx, patches, gwp, G[m + "patch_embed.proj.bias"], B, g, Nt)
        else:
            gwp.copy_(nx.patch_wgrad(dx, patches, None, G[m + "patch_embed.proj.bias"], B, g, Nt)[:, :K])
        cb("embed")
        wg.join()
        S.clear()
