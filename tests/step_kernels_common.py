"""Plain float64 restatements of the train step's non-GEMM kernels -- LayerNorm (csrc/norm.hip), the bilinear resize and its adjoint,
the head output layer and the fused loss (csrc/elementwise.hip) -- each with a per-element error bound built from reference quantities
only, and Python mirrors of the host arithmetic that picks a launch plan.  tests/test_step_kernels_cpu.py ties every restatement to
something independent (F.layer_norm, F.interpolate, autograd, the oracle's loss) and shows that every bound can fail;
tests/test_step_kernels_gpu.py holds the kernels to them.

Notation: u = U32 = 2^-24, the unit roundoff of f32.  One f32 operation returns exact * (1 + e), |e| <= u.  A sum of n terms formed
in ANY order is off by at most n * u * S, S = sum |terms| (every term passes through at most n - 1 additions and
(n - 1) u / (1 - (n - 1) u) <= n u for n <= 4096).  Where an element passes through a known, small number of additions (a tree, a
fixed chain) that number ("depth") replaces n.  Products of two error terms are covered by counting one rounding more than the
expression has.  A bf16 result is the round-to-nearest of the kernel's f32 value v; with |v - ref| <= d that adds half a bf16 ulp at
magnitude |ref| + d (out_bound).  A fused multiply-add only removes a rounding, so contraction never breaks a bound below.

LayerNorm forward (ln_fwd; the kernels: s = sum x, mu = s / D, q = sum (x - mu)^2, rs = rsqrtf(q / D + eps),
y = (x - mu) * rs * g + b):
  mean:  |s^ - s| <= D u S1 (S1 = sum |x|), one rounding of the division:        dmean = u S1 + u |mean|
  var:   with the computed mean m^, sum (x - m^)^2 = D V + D (m^ - mean)^2 exactly.  A term (x - m^)^2 carries 3 roundings (the
         difference enters twice, the product once), the sum D u, the division and the addition of eps one each:
         a = V + eps is known to                                                  da = (D + 6) u (a + dmean^2) + dmean^2
  rstd:  a -> a^-1/2 is monotone, so the error of a moves rstd by at most (a - da)^-1/2 - a^-1/2 (infinite if da >= a: then the
         bound says nothing, honestly); rsqrtf itself is within 2 ulp = 4 u:      drstd = (a - da)^-1/2 - rstd + 4 u (a - da)^-1/2
         A row of variance ~ 0 has rstd ~ eps^-1/2 = 1000 and d rstd / d a = rstd^3 / 2: the bound grows with rstd^3 by itself.
  y:     first order in the two statistics, with |x - mean| + dmean =: xa and rstd + drstd =: ra as the magnitudes so that the
         second-order products are inside; the expression has 4 roundings (difference, two products, the addition of b), 5 are
         counted on the product and one on b:       dy = |g| (ra dmean + xa drstd) + u (5 |g| xa ra + |b|)
  eps is the f32 value the kernel is handed (f32(1e-6) != 1e-6): the reference is evaluated with that value.

LayerNorm backward (ln_bwd), from the mean / rstd tensors GIVEN to the kernel (xh = (x - mu) rs, dg = dy g, s1 = sum dg / D,
s2 = sum dg xh / D, dx = rs (dg - s1 - xh s2) [+ dres]):
  s1: a term has 1 rounding, the sum D u A1 (A1 = sum |dg|), the division one:    ds1 = (D + 1) u A1 / D + u |s1|
  s2: a term has 4 (xh two, dg one, the product one), A2 = sum |dg xh|:            ds2 = (D + 4) u A2 / D + u |s2|
  dx: dg passes 4 roundings (its own, two subtractions, the product with rs), s1 passes 3, xh s2 passes 5 (xh two, the product, a
      subtraction, rs); one more each:         ddx = rs (ds1 + |xh| ds2 + u (5 |dg| + 4 |s1| + 6 |xh s2|))
      with dres one more addition:             + u (rs (|dg| + |s1| + |xh s2|) + |dres|)
  dgamma = sum_rows dy xh: a term has 3 roundings, M terms (+ the prior value):    (M + 3 + acc) u sum |dy xh| (+ |prior|)
  dbeta  = sum_rows dy:                                                            (M + acc) u sum |dy| (+ |prior|)
  The M-term bounds are for small M; the many-block plans are tested with exact inputs instead (n u S would exceed a dropped row).

Bilinear resize (resize_axis, resize_fwd, resize_bwd): output o of an axis reads the source coordinate
  s = scale o, scale = (in - 1) / (out - 1) [0 if out = 1]                         (align_corners)
  s = max(scale (o + 0.5) - 0.5, 0), scale = in / out                              (otherwise)
and blends pixels i0 = min(floor(s), in - 1) and i1 = min(i0 + 1, in - 1) with weights l0 = 1 - l1, l1 = s - i0.  resize_axis states
this as a loop and returns the tap list; the matrices A[o][i] (weights), the adjoint's contributor counts (nonzero weights per column)
and everything else follow from the list.  As a function of s the weight of any pixel is the hat max(0, 1 - |s - i|) (clamped ends
included), which is 1-Lipschitz: a kernel whose f32 coordinate is off by e has every weight off by at most e -- even when floor()
lands on the other side of an integer and the two taps are other pixels than the reference's (their weights are then below e).  Such a
tap lies within one pixel of the reference's, hence the neighbourhood matrix N[o][i] = 1 for i0 - 1 <= i <= i1 + 1.
  The f32 coordinate: scale has one rounding, the product one (align_corners: |s^ - s| <= 2 u s); otherwise o + 0.5 is exact, the
  product carries 2 u scale (o + 0.5) = 2 u (s + 0.5) and the subtraction u s: <= 3 u (s + 0.5).  s - i0 is exact (s >= 0 and
  i0 = floor(s)), 1 - l1 has one rounding of a number <= 1.  COORD_ULPS = 4 half-ulps: every weight is within
        e(o) = COORD_ULPS u (s(o) + 1)
  of the float64 weight (3 u (s + 0.5) + u <= 4 u (s + 1), second order included).
  forward: y = sum wy wx x over 4 taps; a monomial passes 4 roundings (two products, two additions), 5 counted; S = sum wy wx |x|:
        dy = 5 u S + sum (ey N wx + wy ex N + ey ex N N) |x|
  adjoint: dx[i] = sum over the contributing outputs of wy wx dy.  The generic kernel forms (wy wx) dy and adds the pairs in one
  chain, the row-stream kernel adds along x, multiplies by wy and adds along y: a monomial passes at most pairs + 2 roundings either
  way, and the f32 coordinate can give one more contributor per axis than float64 (a weight below e):
        n = (cnt_h + 1) (cnt_w + 1) + 2,   ddx = n u S + the same three coordinate terms with |dy|
  A contributor that the kernel's candidate window misses is NOT an error term: the dropped-contributor mutants must exceed the bound.

Head output layer (head_fwd, head_bwd; z = h . w + bias, out = act(z); g = dout act'; dh = sum_c g w [* (h > 0)]; dw = sum_m g h;
db = sum_m g):
  z:  K products and K additions in some order: (K + 1) u S, S = sum |h w| + |bias|.  tanh and sin are 1-Lipschitz and tanhf / sinf /
      cosf are within ACT_ERR = 2^-21 for results in [-1, 1] (above the 5 ulp of OpenCL's full profile; no fast-math flag is passed)
  g:  none: dout itself.  tanh: dout (1 - y y) from the saved output y: y y is off by u y^2, 1 - . by u |1 - y^2|, the product by
      u |g|:  dg = 3 u |dout| (1 + y^2).  sine: dout cosf(z) from the saved pre-activation:  dg = |dout| ACT_ERR + u |g|
  dh: per channel |w| (dg + 2 u |g|) (product, addition), 3 counted;  dw: sum_m |h| dg + (M + 1) u sum |g h|;
  db: sum dg + M u sum |g|   (small M only; the block plans are tested with integers)

Fused loss (loss; loss_kernel adds a thread's pixels, then a wave (6 levels), the 4 waves of a block (3), multiplies by the
normaliser; loss_reduce_kernel adds ceil(blocks / 256) partials per thread and runs a 256-wide tree (8 levels)):
  depth(term) = terms per pixel * iterations per thread + 6 + 3 + 2 (the normaliser and its product) + ceil(blocks / 256) + 8
  with 2 terms per pixel for the centre and the gradient-map term and 1 for the sdf and the BCE term.  A total is off by
        nrm (sum dterm + depth u (sum |term| + sum dterm))
  where dterm is the error a term is BORN with when it is not relative to the term (3 u |term| otherwise, counted in depth + 3):
  gradient map: e = (G' - G) - (P' - P) carries de = 2 u (|G' - G| + |P' - P|) (three subtractions); |e| is born with de, e^2 with
  2 |e| de + de^2.  BCE: q = 1 / (1 + expf(-p)) is within 6 u q (expf 2 ulp, the addition, the division); logf(q) within
  6 u + 4 u |log q|; log(1 - q) within 6 u q / (1 - q) + u + 4 u |log(1 - q)|.  out5[0] adds the four totals: 3 u sum |totals| more.
  d_center = gscale nrm (2 d | sgn d): 4 roundings, 5 counted (the sign of an f32 difference is exact).
  d_sdf adds up to six components (sdf, two forward and two backward gradient-map terms, BCE) in at most 5 additions and the
  product with gscale; with each component's own roundings: 10 u sum |components|, plus what the components are born with:
  L2: 2 de per gradient-map component; L1: sgn(e) may differ from the reference's by 2 where |e| <= de;
  BCE: (q - t) / max((1 - q) q, 1e-12) * q * (1 - q) re-uses the SAME computed q and 1 - q, so it is (q^ - t) (1 + 5 u):
  nrm (6 u q + 6 u |q - t|).  (The restatement asserts that no clamp of the BCE term is active: |p| < 20.)

Launch-plan mirrors (resize_fwd_plan, resize_bwd_plan, ln_bwd_plan, ln_reduce_deep, head_out_blocks, loss_plan, adam_grid): the host
arithmetic of the launchers, restated so that a test can assert that its shape reaches the plan it names."""
import math

import numpy as np
import torch

from linear_head_common import U32, half_ulp_bf16, worst_ratio          # noqa: F401  (re-exported for the two test files)

ACT_NONE, ACT_TANH, ACT_SINE = 0, 3, 4
ACT_ERR = 2.0 ** -21
COORD_ULPS = 4
INF = float("inf")


def out_bound(ref, delta, dtype):
    """the bound on |stored result - ref| for a kernel whose f32 value is within delta of ref"""
    if dtype == torch.bfloat16:
        return delta + half_ulp_bf16(ref.abs() + delta)
    return delta


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd(x, gamma, beta, eps, var_div=None, mean_skip_last=0):
    """x [M, D], eps the f32 value handed to the kernel -> dict(y, mean, rstd, dy, dmean, drstd): float64 results and f32-level bounds.
    var_div / mean_skip_last build the mutants of the CPU file (variance over D - 1; the last channels left out of the mean's sum)."""
    xd, g, b = x.double(), gamma.double(), beta.double()
    D = xd.shape[-1]
    S1 = xd.abs().sum(-1, keepdim=True)
    if mean_skip_last:
        mean = xd[:, :D - mean_skip_last].sum(-1, keepdim=True) / D
    else:
        mean = xd.sum(-1, keepdim=True) / D
    d = xd - mean
    a = (d * d).sum(-1, keepdim=True) / (var_div or D) + eps
    rstd = a.rsqrt()
    dmean = U32 * S1 + U32 * mean.abs()
    da = (D + 6) * U32 * (a + dmean * dmean) + dmean * dmean
    lo = a - da
    hi_r = torch.where(lo > 0, lo.clamp_min(1e-300).rsqrt(), torch.full_like(a, INF))
    drstd = (hi_r - rstd) + 4 * U32 * hi_r
    xa, ra = d.abs() + dmean, rstd + drstd
    y = d * rstd * g + b
    dy = g.abs() * (ra * dmean + xa * drstd) + U32 * (5 * g.abs() * xa * ra + b.abs())
    return dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], dy=dy, dmean=dmean[:, 0], drstd=drstd[:, 0])


def ln_bwd(dy, x, gamma, mean, rstd, dres=None, prior=None):
    """the backward from the GIVEN mean / rstd.  prior = (dgamma0, dbeta0) for accumulate=True
    -> dict(dx, ddx, dgamma, ddgamma, dbeta, ddbeta)"""
    dyd, xd, g = dy.double(), x.double(), gamma.double()
    M, D = xd.shape
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (xd - mu) * rs
    dg = dyd * g
    A1, A2 = dg.abs().sum(-1, keepdim=True), (dg * xh).abs().sum(-1, keepdim=True)
    s1, s2 = dg.sum(-1, keepdim=True) / D, (dg * xh).sum(-1, keepdim=True) / D
    ds1 = (D + 1) * U32 * A1 / D + U32 * s1.abs()
    ds2 = (D + 4) * U32 * A2 / D + U32 * s2.abs()
    xs = xh * s2
    dx = rs * (dg - s1 - xs)
    ddx = rs.abs() * (ds1 + xh.abs() * ds2 + U32 * (5 * dg.abs() + 4 * s1.abs() + 6 * xs.abs()))
    if dres is not None:
        r = dres.double()
        dx = dx + r
        ddx = ddx + U32 * (rs.abs() * (dg.abs() + s1.abs() + xs.abs()) + r.abs())
    tg = dyd * xh
    dgamma, Sg, dbeta, Sb = tg.sum(0), tg.abs().sum(0), dyd.sum(0), dyd.abs().sum(0)
    acc = 0
    if prior is not None:
        acc = 1
        dgamma, Sg = dgamma + prior[0].double(), Sg + prior[0].double().abs()
        dbeta, Sb = dbeta + prior[1].double(), Sb + prior[1].double().abs()
    return dict(dx=dx, ddx=ddx, dgamma=dgamma, ddgamma=(M + 3 + acc) * U32 * Sg, dbeta=dbeta, ddbeta=(M + acc) * U32 * Sb)


def ln_bwd_plan(M, cus):
    """csrc/norm.hip ln_bwd_blocks + ln_bwd_plan -> (workgroups = partial slabs, rows per workgroup)"""
    nb = min((M + 7) // 8, 1024, 2 * cus)
    rpb = (M + nb - 1) // nb
    return (M + rpb - 1) // rpb, rpb


def ln_reduce_deep(nblocks, phase=0):
    """ln_bwd_reduce, slab phase `phase` of 16 -> (passes of its 8-deep unrolled loop, slabs left to its tail loop)"""
    b, deep = phase, 0
    while b + 16 * 7 < nblocks:
        b, deep = b + 128, deep + 1
    return deep, len(range(b, nblocks, 16))


def device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ------------------------------------------------------------------------------------------------------------- bilinear resize
def resize_axis(n_in, n_out, align, clamp0=True):
    """the tap list of one axis: [(s, i0, l0, i1, l1)] per output index.  clamp0=False is the CPU file's mutant (no clamp at 0)"""
    if align:
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    else:
        scale = n_in / n_out
    taps = []
    for o in range(n_out):
        s = scale * o if align else scale * (o + 0.5) - 0.5
        if not align and clamp0:
            s = max(s, 0.0)
        i0 = min(int(s), n_in - 1)               # int() truncates, as the kernel's cast does (s >= 0 unless the mutant is on)
        i1 = min(i0 + 1, n_in - 1)
        l1 = s - i0
        taps.append((s, i0, 1.0 - l1, i1, l1))
    return taps


def axis_matrices(taps, n_in, device="cpu", drop_first=False):
    """-> (A [out, in] weights, E [out, in] = e(o) on the neighbourhood of o's taps, cnt [in] = contributing outputs per input).
    drop_first is the CPU file's mutant: every input pixel loses its lowest-index contributing output."""
    n_out = len(taps)
    A = torch.zeros((n_out, n_in), dtype=torch.float64)
    E = torch.zeros((n_out, n_in), dtype=torch.float64)
    for o, (s, i0, l0, i1, l1) in enumerate(taps):
        A[o, i0] += l0
        A[o, i1] += l1
        E[o, max(i0 - 1, 0):min(i1 + 1, n_in - 1) + 1] = COORD_ULPS * U32 * (abs(s) + 1.0)
    if drop_first:
        for i in range(n_in):
            nz = torch.nonzero(A[:, i])
            if nz.numel():
                A[int(nz[0]), i] = 0.0
    cnt = (A != 0).sum(0).double()
    return A.to(device), E.to(device), cnt.to(device)


def _apply(L, t, R):
    """sum_h sum_w L[o][h] t[b][h][w][c] R[p][w] -> [b][o][p][c]"""
    return torch.einsum("oh,bhwc,pw->bopc", L, t, R)


def resize_fwd(x, Ho, Wo, align, relu=False, clamp0=True):
    """x [B, Hi, Wi, C] -> (y float64 [B, Ho, Wo, C], the f32-level bound)"""
    _, Hi, Wi, _ = x.shape
    Ah, Eh, _ = axis_matrices(resize_axis(Hi, Ho, align, clamp0), Hi, x.device)
    Aw, Ew, _ = axis_matrices(resize_axis(Wi, Wo, align, clamp0), Wi, x.device)
    xd = x.double()
    xa = xd.abs()
    y = _apply(Ah, xd, Aw)
    bound = 5 * U32 * _apply(Ah.abs(), xa, Aw.abs()) + _apply(Eh, xa, Aw.abs()) + _apply(Ah.abs(), xa, Ew) + _apply(Eh, xa, Ew)
    return (y.clamp_min(0) if relu else y), bound        # max(., 0) is 1-Lipschitz


def resize_bwd(dy, Hi, Wi, align, drop_first=False):
    """dy [B, Ho, Wo, C] -> (dx float64 [B, Hi, Wi, C], the f32-level bound)"""
    _, Ho, Wo, _ = dy.shape
    Ah, Eh, ch = axis_matrices(resize_axis(Hi, Ho, align), Hi, dy.device, drop_first)
    Aw, Ew, cw = axis_matrices(resize_axis(Wi, Wo, align), Wi, dy.device, drop_first)
    d = dy.double()
    da = d.abs()
    T = lambda m: m.t().contiguous()
    dx = _apply(T(Ah), d, T(Aw))
    n = ((ch + 1)[:, None] * (cw + 1)[None, :] + 2)[None, :, :, None]
    bound = n * U32 * _apply(T(Ah), da, T(Aw)) + _apply(T(Eh), da, T(Aw)) + _apply(T(Ah), da, T(Ew)) + _apply(T(Eh), da, T(Ew))
    return dx, bound


def _f32_scale(n_in, n_out, align):
    if align:
        return np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    return np.float32(n_in) / np.float32(n_out)


def _is_bf16(dtype):
    return dtype == torch.bfloat16


def resize_fwd_plan(B, Ho, Wo, C, dtype, ldx=None, ldy=None, gy_cap=0):
    """umr_bilinear_fwd_ex (no plane output) -> dict(kernel, run, gx, gy); ldx / ldy = pixel strides in elements (None: dense)"""
    ldx, ldy, cap = ldx or C, ldy or C, (gy_cap if gy_cap > 0 else 65535)
    nv = 2 if (C % 8 == 0 and ldx % 8 == 0 and ldy % 8 == 0) else 1
    gx = (Wo * (C // (4 * nv)) + 255) // 256
    if nv == 2 and _is_bf16(dtype):
        run = 16
        while run > 2 and B * ((Ho + run - 1) // run) * gx < 2048:
            run = (run + 1) // 2
        runs = B * ((Ho + run - 1) // run)
        return dict(kernel="rowstream", run=run, gx=gx, gy=min(runs, cap), units=runs)
    return dict(kernel="generic%d" % nv, run=1, gx=gx, gy=min(B * Ho, cap), units=B * Ho)


def resize_bwd_plan(B, Hi, Wi, Ho, Wo, C, align, dtype, lddy=None, lddx=None, gy_cap=0):
    """umr_bilinear_bwd_ex -> dict(kernel = 'rowstream6' | 'rowstream8' | 'generic2' | 'generic1', run, gx, gy)"""
    lddy, lddx, cap = lddy or C, lddx or C, (gy_cap if gy_cap > 0 else 65535)
    nv = 2 if (C % 8 == 0 and lddy % 8 == 0 and lddx % 8 == 0) else 1
    gx = (Wi * (C // (4 * nv)) + 255) // 256
    sh, sw = _f32_scale(Hi, Ho, align), _f32_scale(Wi, Wo, align)
    if nv == 2 and _is_bf16(dtype) and sh >= np.float32(0.4) and sw >= np.float32(0.4):
        run = 12
        while run > 2 and B * ((Hi + run - 1) // run) * gx < 2048:
            run = (run + 1) // 2
        runs = B * ((Hi + run - 1) // run)
        six = bool(align) and sw >= np.float32(0.49)
        return dict(kernel="rowstream6" if six else "rowstream8", run=run, gx=gx, gy=min(runs, cap), units=runs)
    return dict(kernel="generic%d" % nv, run=1, gx=gx, gy=min(B * Hi, cap), units=B * Hi)


# ------------------------------------------------------------------------------------------------------------- head output layer
def _act(z, act):
    return torch.tanh(z) if act == ACT_TANH else (torch.sin(z) if act == ACT_SINE else z)


def _nchw(t, B, H, W):
    """[M, Cout] rows (b, y, x) -> [B, Cout, H, W]"""
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    """[B, Cout, H, W] -> [M, Cout]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def head_fwd(h, w, bias, B, H, W, act):
    """h [M, K], w [Cout, K], bias [Cout] -> (out float64 [B, Cout, H, W], bound, z float64 [B, Cout, H, W])"""
    hd, wd, bd = h.double(), w.double(), bias.double()
    K = hd.shape[1]
    z = hd @ wd.t() + bd
    bound = (K + 1) * U32 * (hd.abs() @ wd.abs().t() + bd.abs())
    if act != ACT_NONE:
        bound = bound + ACT_ERR
    return _nchw(_act(z, act), B, H, W), _nchw(bound, B, H, W), _nchw(z, B, H, W)


def head_bwd(h, w, dout, yout, act, relu_mask):
    """dout, yout [B, Cout, H, W] (yout: the saved output for tanh, the saved pre-activation for sine, unused for none)
    -> dict(dh, ddh [M, K], dw, ddw [Cout, K], db, ddb [Cout]) in float64"""
    hd, wd, d = h.double(), w.double(), _rows(dout.double())
    M = hd.shape[0]
    if act == ACT_TANH:
        y = _rows(yout.double())
        g, dg = d * (1 - y * y), 3 * U32 * d.abs() * (1 + y * y)
    elif act == ACT_SINE:
        g = d * torch.cos(_rows(yout.double()))
        dg = d.abs() * ACT_ERR + U32 * g.abs()
    else:
        g, dg = d, torch.zeros_like(d)
    dh, ddh = g @ wd, (dg + 3 * U32 * g.abs()) @ wd.abs()
    if relu_mask:
        keep = (hd > 0).double()
        dh, ddh = dh * keep, ddh * keep
    return dict(dh=dh, ddh=ddh, dw=g.t() @ hd, ddw=dg.t() @ hd.abs() + (M + 1) * U32 * (g.abs().t() @ hd.abs()),
                db=g.sum(0), ddb=dg.sum(0) + M * U32 * g.abs().sum(0))


def head_out_blocks(M):
    """umr_head_out_bwd -> (workgroups, rows per workgroup)"""
    nb = max(1, min((M + 255) // 256, 2048))
    rpb = (M + nb - 1) // nb
    return (M + rpb - 1) // rpb, rpb


def head_fwd_grid(M):
    """umr_head_out_fwd -> (workgroups of 4 waves, rows the busiest wave walks)"""
    g = max(1, min((M + 3) // 4, 16384))
    return g, (M + 4 * g - 1) // (4 * g)


# ------------------------------------------------------------------------------------------------------------- fused loss
def loss_plan(total):
    """umr_objectness_loss -> (blocks of 256 threads, pixels the busiest thread walks)"""
    nb = max(1, min((total + 255) // 256, 1024))
    return nb, (total + nb * 256 - 1) // (nb * 256)


def loss_depth(total, per_pixel):
    nb, iters = loss_plan(total)
    return per_pixel * iters + 6 + 3 + 2 + (nb + 255) // 256 + 8


def adam_grid(n):
    """umr_adam_step / umr_adam_step_hyper -> (blocks of 256 threads, elements the busiest thread walks)"""
    g = max(1, min((n + 255) // 256, 16384))
    return g, (n + g * 256 - 1) // (g * 256)


def _sgn(e):
    return torch.sign(e)


def loss(pc, ps, gc, gs, sal, center_l2, sdf_l2, use_grad, use_bce, gscale=1.0, drop_block=None):
    """pc, gc [B, 2, H, W]; ps, gs, sal [B, 1, H, W] -> dict(out5, dout5 [5]; dpc, ddpc; dps, ddps) in float64.
    out5 = [total, centre, sdf, gradient map, BCE] (a term that is switched off is 0).
    drop_block = k: the CPU file's mutant, the pixels of block k (one pixel per thread: flat indices k*256 .. k*256 + 255) are
    left out of the four totals."""
    pc, ps, gc, gs = pc.double(), ps.double(), gc.double(), gs.double()
    B, _, H, W = pc.shape
    total = B * H * W
    n_c, n_s = 1.0 / (2 * total), 1.0 / total
    n_g = 1.0 / (B * 2 * (H - 1) * (W - 1)) if (H > 1 and W > 1) else 0.0
    keep = torch.ones(total, dtype=torch.float64, device=pc.device)
    if drop_block is not None:
        assert loss_plan(total)[1] == 1
        keep[drop_block * 256:(drop_block + 1) * 256] = 0
    keep = keep.view(B, 1, H, W)
    Z = lambda: torch.zeros((B, 1, H, W), dtype=torch.float64, device=pc.device)

    def total_of(term, born, nrm, per_pixel):
        """-> (total, bound): term / born [B, c, H, W] per element"""
        t, b = (term * keep).sum(), (born * keep).sum()
        s = (term.abs() * keep).sum()
        return nrm * t, nrm * (b + (loss_depth(total, per_pixel) + 3) * U32 * (s + b))

    # centre
    d = pc - gc
    t0, b0 = total_of(d * d if center_l2 else d.abs(), torch.zeros_like(d), n_c, 2)
    dpc = gscale * n_c * (2 * d if center_l2 else _sgn(d))
    ddpc = 5 * U32 * dpc.abs()
    # sdf
    d = ps - gs
    t1, b1 = total_of(d * d if sdf_l2 else d.abs(), torch.zeros_like(d), n_s, 1)
    f = (lambda e: 2 * e) if sdf_l2 else _sgn
    comps = [n_s * f(d).abs()]                    # magnitudes of the components of d_sdf
    g = n_s * f(d)
    gborn = Z()
    t2 = b2 = t3 = b3 = torch.zeros((), dtype=torch.float64, device=pc.device)
    if use_grad and H > 1 and W > 1:
        P, G = ps[:, 0], gs[:, 0]
        gy_, py_ = G[:, 1:, :-1] - G[:, :-1, :-1], P[:, 1:, :-1] - P[:, :-1, :-1]
        gx_, px_ = G[:, :-1, 1:] - G[:, :-1, :-1], P[:, :-1, 1:] - P[:, :-1, :-1]
        ey, ex = gy_ - py_, gx_ - px_
        dey, dex = 2 * U32 * (gy_.abs() + py_.abs()), 2 * U32 * (gx_.abs() + px_.abs())
        term, born = Z(), Z()
        if sdf_l2:
            term[:, 0, :-1, :-1] = ey * ey + ex * ex
            born[:, 0, :-1, :-1] = 2 * ey.abs() * dey + dey * dey + 2 * ex.abs() * dex + dex * dex
            fy, fx, dfy, dfx = 2 * ey, 2 * ex, 2 * dey, 2 * dex
        else:
            term[:, 0, :-1, :-1] = ey.abs() + ex.abs()
            born[:, 0, :-1, :-1] = dey + dex
            fy, fx = _sgn(ey), _sgn(ex)
            dfy, dfx = 2.0 * (ey.abs() <= dey).double(), 2.0 * (ex.abs() <= dex).double()
        t2, b2 = total_of(term, born, n_g, 2)
        for (fv, dfv, sl_here, sl_next) in ((fy, dfy, (slice(None, -1), slice(None, -1)), (slice(1, None), slice(None, -1))),
                                            (fx, dfx, (slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None)))):
            for sl, sign in ((sl_here, 1.0), (sl_next, -1.0)):
                c, cb = Z(), Z()
                c[(slice(None), 0) + sl] = n_g * fv
                cb[(slice(None), 0) + sl] = n_g * dfv
                g = g + sign * c
                comps.append(c.abs())
                gborn = gborn + cb
    if use_bce:
        assert float(ps.abs().max()) < 20, "the clamps of the BCE term must stay inactive for the bound to hold"
        t = sal.double()
        q = torch.sigmoid(ps)
        lq, l1q = torch.log(q), torch.log1p(-q)
        term = -(t * lq + (1 - t) * l1q)
        born = t.abs() * (6 * U32 + 4 * U32 * lq.abs()) + (1 - t).abs() * (6 * U32 * q / (1 - q) + U32 + 4 * U32 * l1q.abs())
        t3, b3 = total_of(term, born, n_s, 1)
        g = g + n_s * (q - t)
        comps.append(n_s * (q - t).abs())
        gborn = gborn + n_s * (6 * U32 * q + 6 * U32 * (q - t).abs())
    dps = gscale * g
    ddps = abs(gscale) * (10 * U32 * sum(comps) + gborn)
    out5 = torch.stack([t0 + t1 + t2 + t3, t0, t1, t2, t3])
    bsum = b0 + b1 + b2 + b3
    dout5 = torch.stack([bsum + 3 * U32 * (t0.abs() + t1.abs() + t2.abs() + t3.abs() + bsum), b0, b1, b2, b3])
    return dict(out5=out5, dout5=dout5, dpc=dpc, ddpc=ddpc, dps=dps, ddps=ddps)


# ------------------------------------------------------------------------------------------------------------- exact inputs
def ints(shape, m, seed, device="cpu"):
    """integers in [-m, m] as f32"""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-m, m + 1, shape, generator=g, device=device).float()


def ln_exact_inputs(M, D, seed, device="cpu"):
    """x in -3..3, dy in -2..2, gamma in quarters of -4..4, mean = 2, rstd = 1/2, dres in -4..4, integer priors: xh is a half-integer,
    dg a quarter; for D = 64 s1 and s2 are multiples of 2^-8 / 2^-9 below 8 and every value of dx's expression is a multiple of 2^-11
    below 32: exact in f32, and a multiple of 1/2 below 2^16 for the parameter sums of up to 2^14 rows"""
    return dict(x=ints((M, D), 3, seed, device), dy=ints((M, D), 2, seed + 1, device), gamma=ints((D,), 4, seed + 2, device) / 4,
                mean=torch.full((M,), 2.0, device=device), rstd=torch.full((M,), 0.5, device=device),
                dres=ints((M, D), 4, seed + 3, device), prior=(ints((D,), 9, seed + 4, device), ints((D,), 9, seed + 5, device)))


def loss_exact_inputs(B, H, W, seed, device="cpu"):
    """targets in halves of -4..4, predictions = target + one of {0, +-1/2, +-1}: every difference, square, and sum of up to 2^21 of
    them is a multiple of 1/4 below 2^22, and the normalisers are powers of two when B H W is one"""
    gc, gs = ints((B, 2, H, W), 4, seed, device) / 2, ints((B, 1, H, W), 4, seed + 1, device) / 2
    pc, ps = gc + ints((B, 2, H, W), 2, seed + 2, device) / 2, gs + ints((B, 1, H, W), 2, seed + 3, device) / 2
    return pc, ps, gc, gs
