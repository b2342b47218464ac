"""What the detector's convolutional heads (mask_head, rpn_head) share on the host: the parameter holder, the argument checks with the
module's name in their messages, the bench tools' launch marks, the pieces of an autograd Function whose backward overwrites a saved
map, the NCHW <-> NHWC permutes and the parameter gradients of a 3x3 convolution on the library's GEMMs."""
import torch

from . import ops, packs

MAX_CHANNELS = 1024
DTYPES = (torch.float32, torch.bfloat16)


class Layer(torch.nn.Module):
    """the parameters of one layer under the reference's names: `weight` (float32, filled by init(weight)), `bias` (zeros)"""

    def __init__(self, weight_shape, init, bias_dim=0):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(weight_shape, dtype=torch.float32))
        self.bias = torch.nn.Parameter(torch.zeros(weight_shape[bias_dim], dtype=torch.float32))
        init(self.weight)


def check_channels(c, subject):
    if not isinstance(c, int) or isinstance(c, bool) or c < 64 or c % 64 or c > MAX_CHANNELS:
        raise ValueError(f"{subject} must be a multiple of 64 up to {MAX_CHANNELS}, got {c!r}")


def check_compute_dtype(compute_dtype, module):
    if compute_dtype not in (None,) + DTYPES:
        raise ValueError(f"{module}: compute_dtype must be None, float32 or bfloat16, got {compute_dtype!r}")


def check_master_copies(params, module):
    for p in params:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"{module}: the parameters are contiguous float32 master copies")


def mark(marks, name):
    """the bench tools time every launch: with a list, a device event after the launch called `name`"""
    if marks is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((name, ev))


def once(ctx, module, stored):
    """the guard of a backward that writes its gradient over the map `stored` it saved (ctx.done = False in the forward)"""
    if ctx.done:
        raise RuntimeError(f"{module}: the backward writes its gradient over the stored {stored}: it runs once per forward")
    ctx.done = True


def masked(grads, need):
    return tuple(g if n else None for g, n in zip(grads, need))


def zeros_like_needed(tensors, need):                            # the gradients of an empty input
    return tuple(torch.zeros_like(t) if n else None for t, n in zip(tensors, need))


def to_nhwc(src, dst):                                           # the recipe of contiguous src [N, C, H, W] -> dst [N, H, W, C]
    N, C, H, W = src.shape
    return src, dst, (N, H, W, C), (C * H * W, W, 1, H * W)


def to_nchw(src, dst):                                           # ... of contiguous src [N, H, W, C] -> dst [N, C, H, W]
    N, C, H, W = dst.shape
    return src, dst, (N, C, H, W), (H * W * C, 1, W * C, C)


def permutes(recipes):
    """the (src, dst, dims, strides) permutes, each cast to its dst's type: one batched launch when there are several"""
    if len(recipes) == 1:
        ops.permute4(*recipes[0])
    elif recipes:
        ops.permute4_batched([r + (0,) for r in recipes])()


def conv3_param_grads(pairs, w, b, marks=None, names=()):
    """The gradients of a 3x3 convolution's parameters over every (dy [M, co], x NHWC) pair it was applied to: the library's weight
    gradient into ONE packed float32 buffer [co][ky][kx][ci] with its bias gradient (umr_gemm_tn adds to both under `accumulate`
    from the second pair on), then the permute to w's layout.  names: a mark after each pair's launch.  Returns (dw, db, packed)."""
    db = torch.empty(b.shape, dtype=torch.float32, device=w.device)
    dwk = None
    for i, (dy, x) in enumerate(pairs):
        dwk = ops.gemm_tn(dy, x, dW=dwk, dbias=db, accumulate=i > 0, conv=1)
        if names:
            mark(marks, names[i])
    return packs._unpack_conv3_grad(dwk, torch.empty_like(w)), db, dwk
