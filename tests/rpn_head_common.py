"""Float64 restatement of the RPN head (unmore_amd/rpn_head.py) for the tests: no test file of its own, imported by test_rpn_head_*.py.
Written from the layer list -- a 3x3 convolution (padding 1) with ReLU, the 1x1 `objectness_logits` and `anchor_deltas` convolutions, the
same weights on every level -- as explicit sums over taps and channels (torch.einsum on shifted maps), NOT on F.conv2d: the CPU tests hold
it against F.conv2d and autograd.  The predictors work on the hidden map of all levels stacked, T [M, C], level after level, row
(n * H + y) * W + x inside a level, as csrc/rpn_head.hip reads it.

Seeded inputs: weights and features are centred, so the hidden pre-activation straddles zero and about half of the ReLU mask is off."""
import math

import torch

U32 = 2.0 ** -24
MUTANTS = ("drop_channel", "swap_bias", "relu_ge", "level_image_offset", "delta_next_anchor")

# the shapes of the kernel tests, (N, C, A, levels): rows that are no multiple of 16 with tiles that straddle images and levels, 1x1 maps;
# the recipe's width with p6's real size; the channel limit with one anchor (11 padded output columns); M exactly 32;
# M = 2112: 17 workgroups of the backward, so the finishing sum's wave 0 adds two partial records
TAIL_SHAPES = [(2, 64, 3, ((5, 7), (3, 4), (1, 1))), (3, 256, 3, ((13, 19), (7, 10))), (1, 1024, 1, ((2, 3),)), (2, 128, 2, ((4, 4),)),
               (2, 64, 3, ((33, 32),))]


# ------------------------------------------------------------------------------------------------ seeded inputs
def make_params(C, A, seed, bias_scale=0.1):
    """float32 state dict under Detectron2's names: the 3x3 weights of std sqrt(2 / (9 C)), the predictors' of std 1 / sqrt(C) (their
    outputs are then O(1), unlike the initial 0.01), biases of std bias_scale (not zero: the bias paths are under test)"""
    g = torch.Generator().manual_seed(seed)
    return {"conv.weight": torch.randn(C, C, 3, 3, generator=g) * math.sqrt(2.0 / (9 * C)),
            "conv.bias": torch.randn(C, generator=g) * bias_scale,
            "objectness_logits.weight": torch.randn(A, C, 1, 1, generator=g) / math.sqrt(C),
            "objectness_logits.bias": torch.randn(A, generator=g) * bias_scale,
            "anchor_deltas.weight": torch.randn(4 * A, C, 1, 1, generator=g) / math.sqrt(C),
            "anchor_deltas.bias": torch.randn(4 * A, generator=g) * bias_scale}


def make_features(N, C, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, C, h, w, generator=g) for h, w in sizes]


def make_grad_maps(N, A, sizes, seed, scale=0.25):
    """(dlogits, ddeltas): both signs, dense"""
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(N, A, h, w, generator=g) * scale for h, w in sizes],
            [torch.randn(N, 4 * A, h, w, generator=g) * scale for h, w in sizes])


def make_hidden(N, C, sizes, seed):
    """a synthetic stacked hidden map: randn().relu(), about half of it zero"""
    M = sum(N * h * w for h, w in sizes)
    return torch.randn(M, C, generator=torch.Generator().manual_seed(seed)).relu()


# ------------------------------------------------------------------------------------------------ layouts
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def stack_rows(maps):
    """per-level NCHW maps [N, K, H, W] -> [M, K], level after level, row (n * H + y) * W + x"""
    return torch.cat([m.permute(0, 2, 3, 1).reshape(-1, m.shape[1]) for m in maps])


def unstack_rows(rows, N, sizes):
    """[M, K] -> the per-level NCHW maps"""
    out, at = [], 0
    for h, w in sizes:
        out.append(rows[at:at + N * h * w].reshape(N, h, w, -1).permute(0, 3, 1, 2).contiguous())
        at += N * h * w
    return out


# ------------------------------------------------------------------------------------------------ the 3x3 convolution with ReLU
def _shifted(x, ky, kx):
    """x [N, C, H, W] -> the map whose (y, x) holds x[y + ky - 1, x + kx - 1], zero outside"""
    N, C, H, W = x.shape
    p = torch.zeros((N, C, H + 2, W + 2), dtype=x.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = x
    return p[:, :, ky:ky + H, kx:kx + W]


def conv3_relu64(x, w, b):
    """relu(b[co] + sum over ci, ky, kx of x[n, ci, y + ky - 1, x + kx - 1] w[co, ci, ky, kx]); float64 NCHW"""
    x, w, b = x.double(), w.double(), b.double()
    z = b.view(1, -1, 1, 1).expand(x.shape[0], w.shape[0], x.shape[2], x.shape[3]).clone()
    for ky in range(3):
        for kx in range(3):
            z += torch.einsum("nchw,oc->nohw", _shifted(x, ky, kx), w[:, :, ky, kx])
    return z.clamp_min(0)


def conv3_adjoint64(x, w, dz):
    """the convolution's adjoint for the gradient dz of its (pre-ReLU) output: (dx, dw, db); float64 NCHW"""
    x, w, dz = x.double(), w.double(), dz.double()
    dw = torch.zeros_like(w)
    dx = torch.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", dz, _shifted(x, ky, kx))
            # dx[y', x'] takes dz[y, x] w[ky, kx] with y' = y + ky - 1: dz shifted the other way
            dx += torch.einsum("nohw,oc->nchw", _shifted(dz, 2 - ky, 2 - kx), w[:, :, ky, kx])
    return dx, dw, dz.sum(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------------ the predictors on the stacked map
def _stacked_weights(wo, bo, wd, bd):
    W = torch.cat([wo.double().reshape(wo.shape[0], -1), wd.double().reshape(wd.shape[0], -1)])
    b = None if bo is None else torch.cat([bo.double().reshape(-1), bd.double().reshape(-1)])
    return W, b


def _image_offset(rows, N, sizes):
    """the mutant's read: the last level's rows taken from the next image"""
    h, w = sizes[-1]
    m = N * h * w
    tail = rows[rows.shape[0] - m:].reshape(N, h * w, -1).roll(-1, 0).reshape(m, -1)
    return torch.cat([rows[:rows.shape[0] - m], tail])


def predict64(T, N, sizes, wo, bo, wd, bd, mutant=None):
    """(logits, deltas): lists of float64 [N, A, H, W] and [N, 4A, H, W]; `mutant`: one of MUTANTS, a wrong kernel"""
    W, b = _stacked_weights(wo, bo, wd, bd)
    A = wo.shape[0]
    T = T.double()
    if mutant == "drop_channel":
        T = T.clone()
        T[:, -1] = 0
    if mutant == "level_image_offset":
        T = _image_offset(T, N, sizes)
    if mutant == "swap_bias":
        b = torch.cat([b[A:], b[:A]])
    out = T @ W.t() + b
    if mutant == "delta_next_anchor":
        out = torch.cat([out[:, :A], out[:, A:].roll(4, 1)], dim=1)
    return unstack_rows(out[:, :A], N, sizes), unstack_rows(out[:, A:], N, sizes)


def predict_abs64(T, N, sizes, wo, bo, wd, bd):
    """the sums of the absolute values of the C + 1 terms of every output, in the outputs' layout"""
    W, b = _stacked_weights(wo, bo, wd, bd)
    A = wo.shape[0]
    s = T.double().abs() @ W.abs().t() + b.abs()
    return unstack_rows(s[:, :A], N, sizes), unstack_rows(s[:, A:], N, sizes)


def predict_bwd64(T, N, sizes, dlogits, ddeltas, wo, wd, mutant=None):
    """(G [M, C], dwo [A, C], dbo [A], dwd [4A, C], dbd [4A]) in float64 for the incoming maps; G = (T > 0) * g W"""
    W, _ = _stacked_weights(wo, None, wd, None)
    A = wo.shape[0]
    T = T.double()
    g = torch.cat([stack_rows([m.double() for m in dlogits]), stack_rows([m.double() for m in ddeltas])], dim=1)
    if mutant == "delta_next_anchor":
        g = torch.cat([g[:, :A], g[:, A:].roll(-4, 1)], dim=1)
    if mutant == "level_image_offset":
        g = _image_offset(g, N, sizes)
    mask = (T >= 0) if mutant == "relu_ge" else (T > 0)
    G = (g @ W) * mask
    dW, db = g.t() @ T, g.sum(0)
    if mutant == "drop_channel":
        G[:, -1] = 0
        dW[:, -1] = 0
    if mutant == "swap_bias":
        db = torch.cat([db[A:], db[:A]])
    return G, dW[:A], db[:A], dW[A:], db[A:]


def predict_bwd_abs64(T, N, sizes, dlogits, ddeltas, wo, wd):
    """the sums of the absolute values of the terms of (G, dwo, dbo, dwd, dbd)"""
    W, _ = _stacked_weights(wo, None, wd, None)
    A = wo.shape[0]
    g = torch.cat([stack_rows([m.double() for m in dlogits]), stack_rows([m.double() for m in ddeltas])], dim=1).abs()
    sW, sb = g.t() @ T.double().abs(), g.sum(0)
    return g @ W.abs(), sW[:A], sb[:A], sW[A:], sb[A:]


# ------------------------------------------------------------------------------------------------ the bounds of the kernel tests
def store_round(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 0.0


def out_allowance(C, scale, ref, out_dtype):
    """a float32 sum of n = C + 1 terms in any order, one ulp per addition: 4 n 2^-24 sum |terms|; a bfloat16 store adds 2^-8 |ref|"""
    return 4 * (C + 1) * U32 * scale + store_round(out_dtype) * ref.abs()


def g_allowance(A, scale, ref, dtype, grads_rounded):
    """the n = 5A sum bound plus one rounding to the compute type; grads_rounded: float32 gradients that the kernel rounds to bfloat16 as
    csrc/rpn_head.hip documents -- 2^-8 sum |terms| more"""
    one = 2.0 ** -8 if dtype == torch.bfloat16 else U32
    return 4 * 5 * A * U32 * scale + one * ref.abs() + (2.0 ** -8 * scale if grads_rounded else 0.0)


def w_allowance(M, scale, grads_rounded):
    return 4 * M * U32 * scale + (2.0 ** -8 * scale if grads_rounded else 0.0)


# ------------------------------------------------------------------------------------------------ the whole head, any float type
def head_chain(features, sd, post=lambda t: t):
    """(logits, deltas) of the head on torch's own conv2d in the features' type; post: applied to every stored tensor (the hidden map and
    the outputs)"""
    import torch.nn.functional as F
    logits, deltas = [], []
    for x in features:
        t = post(F.relu(F.conv2d(x, sd["conv.weight"], sd["conv.bias"], padding=1)))
        logits.append(post(F.conv2d(t, sd["objectness_logits.weight"], sd["objectness_logits.bias"])))
        deltas.append(post(F.conv2d(t, sd["anchor_deltas.weight"], sd["anchor_deltas.bias"])))
    return logits, deltas
