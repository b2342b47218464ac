"""The fp32 parity mode of the engine on the bf16-plane kernels (UMR_F32_X3 / UMR_F32_X3_FAST): its value format and its numerics.

The reference computes in fp32 (object_reasoning.py:74; no autocast in train_objectness_net.py:81,259-260,836), and fp32 is
the mode that carries the 1e-4 / bit-exact-peak contract.  Every f32 value that is a GEMM operand travels as three bf16 planes
(x = h + m + l, lossless; include/umr.h UMR_BF16X3): activations leave the producing kernel already split (GEMM epilogues,
LayerNorm), weights are kept as planes per parameter version, and all Linear / 1x1 / 3x3 layers -- forward, data gradient and
weight gradient -- run on the persistent 256x256 bf16 kernels (csrc/gemm_nt256p.hip X3, csrc/gemm_tn256.hip X3) as six plane-pair
products per f32 product.  Tensors that feed non-GEMM kernels (LayerNorm, attention, resizes, the loss) stay f32.

`XT` carries a value in either or both formats and converts on demand (exactly: split3 / unsplit3), so a layer whose shape the
plane kernels do not take (K not a multiple of 64: the narrow reassemble layers of the small backbones; stride-2 conv; row-gathered
operands) falls back to the 128x128 f32 kernels of csrc/gemm_nt.hip / gemm_tn.hip without the caller noticing.

The launch list itself is engine.Engine.forward / backward, written once for both precision modes: it runs on `X3Numerics` here or
on engine.PlainNumerics, and names values only through mm / wgrad / val and the _f / _any / _drop_f helpers below, which take a
plain tensor as well."""
import torch

from . import _lib as L
from . import ops
from .packs import _ACT, _pack_linear_t


class XT:
    """an [..., n] f32 value as an f32 tensor, as a planes tensor ([..., 3n] bf16), or both.  Views share ONE cell, so a conversion
    made through any view (split3 / unsplit3, exact both ways) is made once."""
    __slots__ = ("cell", "shape")

    def __init__(self, f=None, p=None, _cell=None, _shape=None):
        if _cell is not None:
            self.cell, self.shape = _cell, tuple(_shape)
            return
        assert (f is None) != (p is None) and (f if f is not None else p).is_contiguous()
        self.cell = [f, p]
        self.shape = tuple(f.shape) if f is not None else tuple(p.shape[:-1]) + (p.shape[-1] // 3,)

    @property
    def n(self):
        return self.shape[-1]

    @property
    def f(self):
        return None if self.cell[0] is None else self.cell[0].view(self.shape)

    @property
    def p(self):
        return None if self.cell[1] is None else self.cell[1].view(self.shape[:-1] + (3 * self.shape[-1],))

    def F(self):
        if self.cell[0] is None:
            self.cell[0] = ops.unsplit3(self.cell[1])
        return self.f

    def P(self):
        if self.cell[1] is None:
            self.cell[1] = ops.split3(self.cell[0])
        return self.p

    def drop_f(self):
        """the f32 copy is not needed again (saved activations that only feed plane GEMMs)"""
        if self.cell[1] is not None:
            self.cell[0] = None
        return self

    def any(self):
        """whichever format exists (epilogue operands are taken in either)"""
        return self.f if self.cell[0] is not None else self.p

    def view(self, *shape):
        return XT(_cell=self.cell, _shape=shape)

    def mask_source(self):
        """a tensor whose sign is the value's (oracle/mask_parity.py reads the ReLU decisions from saved activations)"""
        return self.f if self.cell[0] is not None else self.p[..., :self.n]


def _any(t):
    return t.any() if isinstance(t, XT) else t


def _f(t):
    return t.F() if isinstance(t, XT) else t



def _drop_f(t):
    """the f32 copy of a saved activation is not needed again (XT.drop_f); a plain tensor is the only copy there is"""
    if isinstance(t, XT):
        t.drop_f()


class X3Numerics:
    """The fp32 parity mode behind engine.Engine.forward / backward: values are XT, every GEMM goes to the plane kernels where its
    shape allows.  One object per call: e = the Engine (packs, parameters' f32 views, the collapsed-head algebra), P = parameters."""

    def __init__(self, e, P):
        self.e, self.P = e, P

    def val(self, t):
        """an f32 tensor some non-GEMM kernel wrote, as a value of this mode"""
        return XT(f=t)

    def to_dt(self, t):
        """an f32 tensor in the dtype the f32 kernels of this mode take as an operand: itself"""
        return t

    def _x3_ok(self, K, N, conv):
        return conv in (0, 1) and K % 64 == 0 and N % 8 == 0

    def mm(self, A, wname, kind, bias=None, *, conv=0, act=L.ACT_NONE, want="f", mask=None, dgelu=None, aux=None, aux2=None,
           rowbias=None, rows_per_batch=0, c2_mode=0, c2_want="f", out=None, c_remap=None, aux_mod=0):
        """epi(A . W^T) with W = parameter `wname` in layout `kind` (Engine._w kinds; conv = 3x3 mode).  A: XT ([M, K] or NHWC).
        want / c2_want: 'f' (f32) or 'p' (planes) for the output / the second output.  Returns XT, or (XT, XT) with c2_mode."""
        P = self.P
        w = P[wname]
        Kc = A.shape[-1]            # K of a plain GEMM, Cin of a conv
        if kind in ("lin", "lin_a", "lin_b", "c3", "ct_d"):
            N = w.shape[0]
        elif kind == "lin_t":
            N = w[0].numel()        # [N0, K0] or a 1x1 conv weight [co, ci, 1, 1]
        elif kind in ("lin_t_a", "lin_t_b"):
            N = w.shape[1] // 2
        elif kind == "c3_d":
            N = w.shape[1]
        else:                       # "ct": ConvTranspose2d [ci, co, s, s] as a GEMM onto (i, j, co)
            N = w.shape[1] * w.shape[2] * w.shape[3]
        if self._x3_ok(Kc, N, conv):
            Ap = A.P()
            r = ops.gemm_nt_x3(Ap, self.e._wx3(P, wname, kind), bias, act=act, conv=conv, out_planes=(want == "p"), out=out,
                               mask=_any(mask), dgelu=_any(dgelu), aux=_any(aux), aux2=_any(aux2), rowbias=rowbias,
                               rows_per_batch=rows_per_batch, c2_mode=c2_mode, c2_planes=(c2_want == "p"), c_remap=c_remap, aux_mod=aux_mod)
            wrap = lambda t: XT(p=t) if t.dtype == torch.bfloat16 else XT(f=t)
            return (wrap(r[0]), wrap(r[1])) if c2_mode else wrap(r)
        # shapes the plane kernels do not take: the 128x128 f32 kernels (in-register splits), f32 operands
        Wf = self._w_f32(wname, kind)
        a_t = mask if mask is not None else (dgelu if dgelu is not None else aux)
        r = ops.gemm_nt(A.F(), Wf, bias, out=out, aux=_f(a_t), aux2=_f(aux2), rowbias=rowbias, rows_per_batch=rows_per_batch, act=act,
                        mask_relu=mask is not None, mask_dgelu=dgelu is not None, c2_mode=c2_mode, conv=conv, c_remap=c_remap, aux_mod=aux_mod)
        return (XT(f=r[0]), XT(f=r[1])) if c2_mode else XT(f=r)

    def _w_f32(self, name, kind):
        """f32 kernel-layout weights for the fallback path (the halves of the readout weight are slices of the full pack)"""
        e, P = self.e, self.P
        if kind in ("lin_a", "lin_b"):
            w = e._w(P, name, "lin")
            D = w.shape[1] // 2
            return w[:, :D] if kind == "lin_a" else w[:, D:]
        if kind in ("lin_t_a", "lin_t_b"):
            w = P[name].detach()
            D = w.shape[1] // 2
            half = w[:, :D] if kind == "lin_t_a" else w[:, D:]
            return e.cache.get((name, kind, torch.float32), P[name], lambda: _pack_linear_t(half, torch.float32))
        return e._w(P, name, kind)

    def wgrad(self, dY, X, dW, dbias=None, *, conv=0, accumulate=False, wg=None, then=None):
        """dW (+)= dY^T X (X NHWC with conv); plane kernel where it applies (N, K multiples of 8, no stride-2 conv).
        wg: engine.WgradStream -- the launch (and `then(dW)`, e.g. the unpacking of a conv gradient) goes to the weight-gradient
        stream; the operand conversions stay on the main stream, where the data-gradient GEMMs share them."""
        N = dY.shape[-1]
        Kc = X.shape[-1]
        x3 = conv in (0, 1) and N % 8 == 0 and Kc % 8 == 0
        a, b = (dY.P().reshape(-1, 3 * N), X.P()) if x3 else (dY.F().reshape(-1, N), X.F())
        res = []

        def launch():
            r = ops.gemm_tn(a, b, dW=dW, dbias=dbias, conv=conv, accumulate=accumulate, x3=x3)
            if then is not None:
                then(r)
            res.append(r)
        if wg is None or not wg.on:
            launch()
            return res[0]
        wg.run(launch, a, b)
        return None

    # ------------------------------------------------------------------ the steps of the schedule that are this mode's own
    def layernorm(self, x, gamma, beta):
        """the normalised rows leave the kernel as planes: they only feed a GEMM"""
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, planes=True)
        return XT(p=y), mean, rstd

    def readout(self, tok, wname, bias, save, B, g, Nt, D):
        """ProjectReadout (vit.py:86-90) on the hooked tokens [B*Nt, D]: the token rows are compacted once into planes (kept for
        the weight gradient), the class-token half of the weight [D, 2D] adds a per-image row bias"""
        # class-token half + bias: B rows (tiny): the 128x128 f32 kernel on the parameter itself
        rb = ops.gemm_nt(tok, self.e._w(self.P, wname, "lin")[:, D:], bias, M=B, lda=Nt * D, out_f32=True)
        tokp = XT(p=ops.split3(tok, remap=(g, Nt, 1)))     # the token rows without the class-token rows, compact
        if save:
            r, rpre = self.mm(tokp, wname, "lin_a", None, rowbias=rb, rows_per_batch=g, act=L.ACT_GELU, c2_mode=2, want="p")
        else:
            r, rpre = self.mm(tokp, wname, "lin_a", None, rowbias=rb, rows_per_batch=g, act=L.ACT_GELU, want="p"), None
        return dict(r=r, rpre=rpre, tokp=tokp)

    def readout_wgrad(self, d_rpre, rs, tok, dW, B, g, Nt):
        """token half of the readout weight's gradient, from the compact rows the forward kept"""
        self.wgrad(d_rpre, rs["tokp"], dW)

    def hook_grad(self, d_rpre, sB, wname, dx, B, g, Nt, D):
        """the readout's data gradient added into the token gradient dx [B*Nt, D] (created here at the last hook)"""
        if dx is None:
            dx = torch.zeros((B * Nt, D), dtype=torch.float32, device=sB.device)
        self.mm(d_rpre, wname, "lin_t_a", None, out=dx, aux=dx, c_remap=(g, Nt, 1))
        cls_rows = dx.view(B, Nt * D)[:, :D]  # token 0 of every image: row stride Nt*D
        ops.gemm_nt(sB, self._w_f32(wname, "lin_t_b"), None, out=cls_rows, aux=cls_rows)
        return dx

    def head_resize(self, h1l, shape_low, H, W, relu):
        """resize(W1 path + b1), then the ReLU: written straight as the planes the 3x3 conv stages"""
        h1 = ops.bilinear_fwd(h1l.F().view(*shape_low, -1), H, W, True, relu=relu, planes=True)
        return XT(p=h1).view(shape_low[0] * H * W, h1l.n)

    def head_tail(self, h2, w3name, b3, w4, b4, act, final, keep, pre, B, H, W):
        """third and output layer of a factored head: (out, h3 or None, pre-activation of the output or None)"""
        if not keep:
            # the 1024 -> {1,2} output layer rides in the epilogue of the layer that produces its input: h3 is never stored
            parts = ops.gemm_nt_x3(h2.P(), self.e._wx3(self.P, w3name, "lin"), b3, act=act, red_w=w4.contiguous())
            return ops.head_out_finish(parts, b4, B, H, W, final), None, None
        h3 = self.mm(h2, w3name, "lin", b3, act=act).F()     # f32: the output layer and its backward read the values
        out = ops.head_out_fwd(h3, w4, b4, B, H, W, final)
        return out, h3, (ops.head_out_fwd(h3, w4, b4, B, H, W, L.ACT_NONE) if pre else None)

    def heads_backward(self, S, d_center, d_sdf, G, wgrad_lin, wgrad_c3, done):
        """Backward of both heads, head by head: each adds its share to the gradient of the feature map (or, when the first layer
        ran before the final resize -- engine._COMMUTE_RESIZE -- of the small map).  done() closes the stage.  Returns that gradient
        as the value the last fusion block's backward reads."""
        e, P, mm = self.e, self.P, self.mm
        B, H, W = S["B"], S["H"], S["W"]
        dev = d_center.device
        M = B * H * W
        lowres = S.get("path") is not None
        feat = S["feat"]
        feat2 = None if lowres else feat.view(M, 256)
        if lowres:
            pathx = S["path"]
            nbp, php, pwp = pathx.shape[0], pathx.shape[1], pathx.shape[2]
            Ml = nbp * php * pwp
            pl = pathx.view(Ml, 256)
        dfeat = None          # f32 [M, 256] (lowres: the gradient of the map before the resize, [Ml, 256])
        for hi, (name, lay, dout) in enumerate((("center_field_prediction_head", e.center_layout, d_center),
                                                ("sdf_prediction_head", e.sdf_layout, d_sdf))):
            hs = S["heads"][hi]
            idx = lay["conv_idx"]
            if lowres and hs.get("algebraic"):
                # the head's two reductions as products on the small map (csrc/linear_head.hip, lh_shift9_kernel)
                if "u" not in hs:
                    hs["u"], hs["Vc"], hs["Kw"], _ = e._linear_head_weights(P, name, idx, dev)
                s9, nd = ops.linear_head_shift9(dout.contiguous(), hs["out"], hs["act"], torch.float32)
                E = ops.bilinear_bwd(s9, php, pwp, True).view(Ml, 16)
                del s9
                gm = ops.gemm_tn(E, pl.F())
                e._linear_head_algebra(P, name, idx, hs, gm[:9].reshape(-1), nd[:9], nd[9:10], G)
                kwt = torch.zeros((256, 16), dtype=torch.float32, device=dev)
                kwt[:, :9].copy_(hs["Kw"].view(9, 256).t())
                dfeat = ops.gemm_nt(E, kwt, None) if dfeat is None else ops.gemm_nt(E, kwt, None, aux=dfeat, out=dfeat)
                continue
            if hs.get("collapsed") or hs.get("algebraic"):
                dfeat = e._linear_head_backward(P, name, idx, feat.F().view(B, H, W, 256), hs, dout, dfeat, G)
                continue
            relu = lay["relu"]
            w4 = e._f32(P, f"{name}.{idx[3]}.weight")
            dh3 = XT(f=ops.head_out_bwd(hs["h3"], w4.reshape(w4.shape[0], -1), dout.contiguous(), hs["out"], _ACT[lay["final"]], relu,
                                        G[f"{name}.{idx[3]}.weight"].view(w4.shape[0], -1), G[f"{name}.{idx[3]}.bias"]))
            hs["h3"] = None
            wgrad_lin(f"{name}.{idx[2]}.weight", dh3, hs["h2"], f"{name}.{idx[2]}.bias")
            dh2 = mm(dh3, f"{name}.{idx[2]}.weight", "lin_t", None, mask=(hs["h2"] if relu else None), want="p")
            del dh3
            h1 = hs["h1"].view(B, H, W, 512)
            wgrad_c3(f"{name}.{idx[1]}.weight", dh2, h1, f"{name}.{idx[1]}.bias")
            hs["h2"] = None
            dh1 = mm(dh2.view(B, H, W, 512), f"{name}.{idx[1]}.weight", "c3_d", None, conv=1, mask=(hs["h1"] if relu else None),
                     want=("f" if lowres else "p"))
            del dh2
            hs["h1"] = None
            if lowres:
                dh1 = XT(f=ops.bilinear_bwd(dh1.F().view(B, H, W, dh1.n), php, pwp, True)).view(Ml, dh1.n)
            wgrad_lin(f"{name}.{idx[0]}.weight", dh1, (pl if lowres else feat2), f"{name}.{idx[0]}.bias")
            if dfeat is None:
                dfeat = mm(dh1, f"{name}.{idx[0]}.weight", "lin_t", None).F()
            else:
                dfeat = mm(dh1, f"{name}.{idx[0]}.weight", "lin_t", None, aux=dfeat).F()
            del dh1
        S["feat"] = None
        S["path"] = None
        done()
        if lowres:
            return XT(f=dfeat.view(nbp, php, pwp, 256))
        ph, pw = S["path1_hw"]
        return XT(f=ops.bilinear_bwd(dfeat.view(B, H, W, 256), ph, pw, True))

    def patch_wgrad(self, dx, patches, dW, dbias, B, g, Nt):
        """gradient of the patch-embedding weight (dW None: returned, in the padded layout of `patches`)"""
        dxp = XT(p=ops.split3(dx, remap=(g, Nt, 1)))      # token gradients without the class-token rows
        return self.wgrad(dxp, patches, dW, dbias)
