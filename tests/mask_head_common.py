"""Float64 restatement of the detector's mask head (unmore_amd/mask_head.py) for the tests: no test file of its own, imported by
test_mask_head_*.py.  Written from the layer list -- 3x3 convolutions with ReLU, a 2x2 stride-2 ConvTranspose2d with ReLU, a 1x1
predictor -- on torch's own F.conv2d, F.conv_transpose2d, relu and sigmoid, plus the GEMM-form pieces the per-layer checks need:
the predictor on the deconvolution GEMM's output D [R*S*S, 4C] (row (r*S + y)*S + x, column (2*ky + kx)*C + co) and its backward.

Seeded inputs: weights and features are centred, so every pre-activation straddles zero and about half of every ReLU mask is off;
the weights are scaled by sqrt(2 / fan_in), which keeps the activations' scale from layer to layer."""
import math

import torch
import torch.nn.functional as F

def make_params(in_channels, conv_dims, seed, bias_scale=0.1):
    """float32 state dict under the reference's names: centred normal weights of std sqrt(2 / fan_in), the predictor's of std
    1 / sqrt(C) (its logits are then O(1), unlike the reference's initial 0.001), biases of std bias_scale (not zero: the bias
    paths are under test)"""
    g = torch.Generator().manual_seed(seed)
    sd, cur = {}, in_channels
    for k, c in enumerate(conv_dims[:-1]):
        sd[f"mask_fcn{k + 1}.weight"] = torch.randn(c, cur, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cur))
        sd[f"mask_fcn{k + 1}.bias"] = torch.randn(c, generator=g) * bias_scale
        cur = c
    c5 = conv_dims[-1]
    sd["deconv.weight"] = torch.randn(cur, c5, 2, 2, generator=g) * math.sqrt(2.0 / cur)
    sd["deconv.bias"] = torch.randn(c5, generator=g) * bias_scale
    sd["predictor.weight"] = torch.randn(1, c5, 1, 1, generator=g) / math.sqrt(c5)
    sd["predictor.bias"] = torch.randn(1, generator=g) * bias_scale
    return sd


def make_features(R, C, S, seed):
    return torch.randn(R, C, S, S, generator=torch.Generator().manual_seed(seed))


def make_dlogits(R, S, seed, scale=0.25):
    """both signs; the scale keeps the weight gradients, sums over R*S*S positions, at O(1)"""
    return torch.randn(R, 1, 2 * S, 2 * S, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ the layers, NCHW, any float type
def conv_relu(a, w, b):
    return F.relu(F.conv2d(a, w, b, padding=1))


def deconv_relu(a, w, b):
    return F.relu(F.conv_transpose2d(a, w, b, stride=2))


def head_logits(x, sd, nconv, post=lambda t: t):
    """the head's logits [R,1,2S,2S] in x's type from a state dict of that type; post: applied to every layer's output"""
    a = x
    for k in range(nconv):
        a = post(conv_relu(a, sd[f"mask_fcn{k + 1}.weight"], sd[f"mask_fcn{k + 1}.bias"]))
    a = post(deconv_relu(a, sd["deconv.weight"], sd["deconv.bias"]))
    return post(F.conv2d(a, sd["predictor.weight"], sd["predictor.bias"]))


def weighted_bce(logits, targets, weights):
    """mean over R*M*M of w_r * binary_cross_entropy_with_logits(x, t), in the logits' type"""
    t = targets.to(logits.dtype).view_as(logits)
    terms = F.binary_cross_entropy_with_logits(logits, t, reduction="none")
    return (terms * weights.to(logits.dtype).view(-1, 1, 1, 1)).mean()


class _RoundTo(torch.autograd.Function):
    """the value rounded to `dtype` and widened again, forward and backward: what storing a layer's output and its gradient in
    the compute type does"""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.to(dtype).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def round_to(t, dtype):
    return _RoundTo.apply(t, dtype)


# ------------------------------------------------------------------------------------------------ layouts
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def cols_to_map(D, R, S):
    """[R*S*S, 4C] in the (ky,kx,co) column order -> NCHW [R,C,2S,2S]"""
    C = D.shape[1] // 4
    return D.reshape(R, S, S, 2, 2, C).permute(0, 5, 1, 3, 2, 4).reshape(R, C, 2 * S, 2 * S)


def map_to_cols(m, R, S):
    """NCHW [R,C,2S,2S] -> [R*S*S, 4C]"""
    C = m.shape[1]
    return m.reshape(R, C, S, 2, S, 2).permute(0, 2, 4, 3, 5, 1).reshape(R * S * S, 4 * C)


def _taps(v, R, S):
    """[R,1,2S,2S] -> [R*S*S, 4], column 2*ky + kx"""
    return v.reshape(R, S, 2, S, 2).permute(0, 1, 3, 2, 4).reshape(R * S * S, 4)


# ------------------------------------------------------------------------------------------------ the tail in GEMM form
def tail_logits64(D, wp, bp, S):
    """float64 [R,1,2S,2S]: bp + sum_co D[m,(ky,kx,co)] * wp[co] at (r, 2y + ky, 2x + kx)"""
    M, C = D.shape[0], D.shape[1] // 4
    R = M // (S * S)
    dots = (D.double().reshape(M, 4, C) * wp.double().reshape(1, 1, C)).sum(-1) + bp.double().reshape(())
    return dots.reshape(R, S, S, 2, 2).permute(0, 1, 3, 2, 4).reshape(R, 1, 2 * S, 2 * S)


def tail_abs64(D, wp, bp, S):
    """|bp| + sum_co |D * wp| per logit, float64 [R,1,2S,2S]: what the error bound of the float32 sum scales with"""
    return tail_logits64(D.double().abs(), wp.double().abs(), bp.double().abs(), S)


def tail_bwd(D, dlogits, wp):
    """(G, dwp, dbp) of the predictor's backward on D [R*S*S, 4C]: G in D's type = D > 0 ? dlogit * wp[co] : 0 with the product formed
    in float32 and rounded once; dwp float64 [C] = sum over rows and taps of dlogit * D, dbp float64 = sum of dlogits"""
    M, C = D.shape[0], D.shape[1] // 4
    R = dlogits.shape[0]
    S = dlogits.shape[-1] // 2
    assert M == R * S * S
    taps = _taps(dlogits, R, S)                                                      # [M, 4]
    prod = taps.float().reshape(M, 4, 1) * wp.float().reshape(1, 1, C)             # float32 products
    G = torch.where(D.reshape(M, 4, C) > 0, prod, torch.zeros((), dtype=torch.float32, device=D.device)).to(D.dtype).reshape(M, 4 * C)
    dwp = (taps.double().reshape(M, 4, 1) * D.double().reshape(M, 4, C)).sum(dim=(0, 1))
    return G, dwp, dlogits.double().sum()


def tail_bwd_abs(D, dlogits):
    """sum |dlogit * D| per channel and sum |dlogit|: the scales of the two sums' error bounds"""
    M, C = D.shape[0], D.shape[1] // 4
    R, S = dlogits.shape[0], dlogits.shape[-1] // 2
    taps = _taps(dlogits, R, S).double().abs()
    return (taps.reshape(M, 4, 1) * D.double().abs().reshape(M, 4, C)).sum(dim=(0, 1)), dlogits.double().abs().sum()


# ------------------------------------------------------------------------------------------------ layer adjoints, float64
def conv_adjoint64(a_in, w, b, dz, mask_of=None):
    """a 3x3 convolution's adjoint: a_in NHWC (the stored input), dz NHWC (the gradient of its pre-activation) -> (d a_in NHWC -- times
    (mask_of > 0) when given: the gradient of the pre-activation below --, dw, db), float64"""
    a = nchw(a_in.double()).requires_grad_(True)
    w64, b64 = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    F.conv2d(a, w64, b64, padding=1).backward(nchw(dz.double()))
    da = nhwc(a.grad)
    if mask_of is not None:
        da = da * (mask_of.double() > 0)
    return da, w64.grad, b64.grad


def deconv_adjoint64(a_in, w, b, G, mask_of=None):
    """the deconvolution's adjoint: a_in NHWC [R,S,S,ci], G [R*S*S, 4*co] (the gradient of its pre-activation in the column order) ->
    (d a_in NHWC, masked as above, dw [ci,co,2,2], db), float64"""
    R, S = a_in.shape[0], a_in.shape[1]
    a = nchw(a_in.double()).requires_grad_(True)
    w64, b64 = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    F.conv_transpose2d(a, w64, b64, stride=2).backward(cols_to_map(G.double(), R, S))
    da = nhwc(a.grad)
    if mask_of is not None:
        da = da * (mask_of.double() > 0)
    return da, w64.grad, b64.grad


# ------------------------------------------------------------------------------------------------ ops.permute4 on the host
def permute4_host(src, dst, dst_dims, src_strides, src_offset=0, accumulate=False):
    """ops.permute4's definition with torch.as_strided (no negative strides): lets the CPU tests run packs' own packers"""
    assert not accumulate and all(s >= 0 for s in src_strides)
    view = torch.as_strided(src.detach(), tuple(dst_dims), tuple(src_strides), src.storage_offset() + src_offset)
    dst.copy_(view.reshape(dst.shape).to(dst.dtype))
    return dst
