"""Plain float64 restatement of the collapsed head's kernels (csrc/linear_head.hip) and of the two small helpers whose
indexing is all they are (small_gemm, segsum): loops over images and taps, zero-padded slices, nothing else.

With off_t = (t // 3 - 1, t % 3 - 1) and everything outside the image zero (the header comment of linear_head.hip):
    z(p)     = sum_{t: p + off_t inside} (kw[t] . x(p + off_t) + tb[t]) + tb[9],   out = act(z)
    g        = dout * act'(yout)          (tanh: 1 - y^2 from the SAVED OUTPUT; identity otherwise)
    dx(p)[c] (+)= sum_t kw[t][c] g(p - off_t)
    G[t][c]  = sum_q x(q)[c] g(q - off_t),   n[t] = sum_q [q - off_t inside] g(q - off_t),   D = sum g

Every function works in float64 on the device of its inputs and also returns, per output element,
    S = sum |terms|   and   n = the number of terms,
the two quantities of the order-independent worst case of f32 summation |computed - exact| <= n * 2^-24 * S.

What a "term" is: a monomial of the inputs.  For act none a term of dx / G / n is kw*g or x*g with g = dout.  For tanh
g = dout - dout*y^2 is two monomials, so every such term counts twice and contributes |.|*|dout|*(1 + y^2) to S: the rounding of
y*y is an ABSOLUTE error of 2^-25 |dout| y^2 in g, not one relative to g, and this is the S that covers it.  A monomial passes
through at most 3 roundings while g is formed, one for its product and one per addition that joins it to the rest (at most
terms - 1, whatever the order), so the bound holds whenever an element has at least 3 terms before doubling; elements without any
term are exactly zero on both sides.  tests/test_head_kernels_cpu.py checks all of this file against float64 conv2d / autograd."""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
ACT_NONE, ACT_TANH, ACT_SINE = 0, 3, 4     # include/umr.h: UMR_ACT_NONE, UMR_ACT_TANH; 4 = sine (ops.ACT_SINE)


def off(t):
    return t // 3 - 1, t % 3 - 1


def shifted(a, dy, dx):
    """s(p) = a(p + (dy, dx)), zero where p + (dy, dx) is outside the image; a is [H, W] or [H, W, C]"""
    H, W = a.shape[0], a.shape[1]
    p = F.pad(a, (1, 1, 1, 1) if a.dim() == 2 else (0, 0, 1, 1, 1, 1))
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def act_apply(z, act):
    return torch.tanh(z) if act == ACT_TANH else (torch.sin(z) if act == ACT_SINE else z)


def _g(dout_b, yout_b, act):
    """(g, sum of |monomials| of g, monomials per g) of one image, [H, W]"""
    d = dout_b.double()
    if act == ACT_TANH:
        y = yout_b.double()
        return d * (1.0 - y * y), d.abs() * (1.0 + y * y), 2
    assert act == ACT_NONE, "the backward exists for tanh and none only"
    return d, d.abs(), 1


def fwd(x, kw, tb, act):
    """x [B, H, W, C], kw [9, C], tb [10] -> (out [B, 1, H, W], S, n), S and n of the pre-activation sum"""
    B, H, W, C = x.shape
    kw, tb = kw.double().view(9, C), tb.double()
    out = torch.zeros((B, 1, H, W), dtype=torch.float64, device=x.device)
    S, n = torch.zeros_like(out), torch.zeros_like(out)
    one = torch.ones((H, W), dtype=torch.float64, device=x.device)
    for b in range(B):
        xb = x[b].double()
        z, s, cnt = tb[9] * one, tb[9].abs() * one, one.clone()
        for t in range(9):
            dy, dx = off(t)
            xs, ins = shifted(xb, dy, dx), shifted(one, dy, dx)
            z = z + (xs * kw[t]).sum(-1) + tb[t] * ins
            s = s + (xs.abs() * kw[t].abs()).sum(-1) + tb[t].abs() * ins
            cnt = cnt + (C + 1) * ins
        out[b, 0], S[b, 0], n[b, 0] = act_apply(z, act), s, cnt
    return out, S, n


def bwd_data(dout, yout, kw, act, prior=None):
    """dout, yout [B, 1, H, W] (yout may be None for act none), kw [9, C], prior [B, H, W, C] or None -> (dx [B, H, W, C], S, n)"""
    B, _, H, W = dout.shape
    kw = kw.double().view(9, -1)
    C = kw.shape[1]
    dx = torch.zeros((B, H, W, C), dtype=torch.float64, device=dout.device)
    S = torch.zeros_like(dx)
    mono = 1
    for b in range(B):
        g, ga, mono = _g(dout[b, 0], None if yout is None else yout[b, 0], act)
        acc = torch.zeros((H, W, C), dtype=torch.float64, device=dout.device) if prior is None else prior[b].double().clone()
        s = acc.abs()
        for t in range(9):
            dy, dx_ = off(t)
            acc = acc + shifted(g, -dy, -dx_)[..., None] * kw[t]
            s = s + shifted(ga, -dy, -dx_)[..., None] * kw[t].abs()
        dx[b], S[b] = acc, s
    return dx, S, 9 * mono + (prior is not None)


def bwd_weight(x, dout, yout, act):
    """-> (R, S, n), each [9 * C + 10] laid out as the kernel's result [G (9, C) | n (9) | D (1)]"""
    B, H, W, C = x.shape
    dev = x.device
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    G, SG, nt, Sn, cnt, D, SD = z(9, C), z(9, C), z(9), z(9), z(9), z(1), z(1)
    one = torch.ones((H, W), dtype=torch.float64, device=dev)
    mono = 1
    for b in range(B):
        xb = x[b].double()
        xa = xb.abs()
        g, ga, mono = _g(dout[b, 0], None if yout is None else yout[b, 0], act)
        for t in range(9):
            dy, dx = off(t)
            gs, gas = shifted(g, -dy, -dx), shifted(ga, -dy, -dx)
            G[t] += (xb * gs[..., None]).sum((0, 1))
            SG[t] += (xa * gas[..., None]).sum((0, 1))
            nt[t] += gs.sum()
            Sn[t] += gas.sum()
            cnt[t] += shifted(one, -dy, -dx).sum()
        D += g.sum()
        SD += ga.sum()
    R = torch.cat([G.reshape(-1), nt, D])
    S = torch.cat([SG.reshape(-1), Sn, SD])
    n = torch.cat([cnt[:, None].expand(9, C).reshape(-1), cnt, z(1) + B * H * W]) * mono
    return R, S, n


def small_gemm(A, B, Cprior, M, N, K, sa, sb, sc, accumulate=False):
    """C[i*sc[0] + j*sc[1]] (=|+=) sum_k A[i*sa[0] + k*sa[1]] * B[k*sb[0] + j*sb[1]] on flat tensors, element strides.
    -> (the whole flat C after the call, the flat indices [M, N] it wrote, S [M, N], n)"""
    i = torch.arange(M).view(M, 1, 1)
    j = torch.arange(N).view(1, N, 1)
    k = torch.arange(K).view(1, 1, K)
    a = A.double().reshape(-1)[i * sa[0] + k * sa[1]]          # [M, 1, K]
    b = B.double().reshape(-1)[k * sb[0] + j * sb[1]]          # [1, N, K]
    terms = a * b                                              # [M, N, K]
    ic = (i * sc[0] + j * sc[1]).view(M, N)
    assert ic.unique().numel() == M * N, "the result elements must be distinct"
    out = Cprior.double().reshape(-1).clone()
    s, S = terms.sum(-1), terms.abs().sum(-1)
    if accumulate:
        s, S = s + out[ic], S + out[ic].abs()
    out[ic] = s
    return out, ic, S, K + int(accumulate)


def segsum(x, R, reps, rep_stride, seg_stride, C, prior=None):
    """out[r][c] (+= prior) = sum_{k < reps} x[r*seg_stride + k*rep_stride + c] -> (out [R, C], S, n)"""
    r = torch.arange(R).view(R, 1, 1)
    k = torch.arange(reps).view(1, reps, 1)
    c = torch.arange(C).view(1, 1, C)
    v = x.double().reshape(-1)[r * seg_stride + k * rep_stride + c]     # [R, reps, C]
    out, S = v.sum(1), v.abs().sum(1)
    if prior is not None:
        out, S = out + prior.double().view(R, C), S + prior.double().view(R, C).abs()
    return out, S, reps + (prior is not None)


def half_ulp_bf16(v):
    """half a unit in the last place of bf16 (8 significant bits) at the magnitude of v; 0 at v = 0"""
    _, e = torch.frexp(v.abs())                               # |v| = m * 2^e, m in [0.5, 1)
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 9))


def worst_ratio(out, ref, bound):
    """max of |out - ref| / bound over the elements with a positive bound; elements whose bound is 0 must be equal.
    -> (ratio, number of elements over their bound)"""
    err = (out.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    pos = bound > 0
    bad = int((err > bound).sum())
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return ratio, bad
