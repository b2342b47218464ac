"""Plain float64 restatements of the existence classifier's hand-written kernels -- the training-mode BatchNorm (statistics, apply,
backward), the max-pool and its gradient, the BCE loss (csrc/clf_train.hip), the stem's im2col and the BatchNorm fold
(csrc/classifier.hip) -- each with a per-element error bound built from float64 reference quantities and the inputs only, and a Python
mirror of the host arithmetic that picks the reductions' launch plan.  tests/test_clf_kernels_cpu.py ties every restatement to
something independent (F.batch_norm, F.max_pool2d, F.binary_cross_entropy, F.unfold and autograd) and shows that every bound can fail;
tests/test_clf_kernels_gpu.py holds the kernels to them.

Notation and the rules of counting are those of tests/step_kernels_common.py: u = U32 = 2^-24; one f32 operation returns
exact * (1 + e), |e| <= u; a term that passes through n >= 2 roundings is charged (n + 1) u so that the products of error terms are
inside; a term that passes through `depth` additions of a fixed reduction is charged depth * u; a fused multiply-add only removes a
rounding; a bf16 result adds half a bf16 ulp at the magnitude |ref| + delta (out_bound).

The column reductions (bn_plan).  The rows are split into `chunks` chunks of rpc rows.  In a chunk a thread adds every 16th row in a
chain (ceil(rpc / 16) additions), the 16 row lanes of the block are added in a chain (16), lane l of the final kernel's wave adds the
chunks l, l + 64, ... in a chain (ceil(chunks / 64)) and a xor tree combines the 64 lanes (6):
        depth = ceil(rpc / 16) + 16 + ceil(chunks / 64) + 6

Statistics (bn_stats; bn_stats_partial_kernel / bn_stats_final_kernel: k = z[0, c], v = z - k, s1 = sum v, s2 = sum v^2, d = s1 / n,
m2 = max(s2 - s1 d, 0), mean = k + d, rstd = 1 / sqrtf(m2 / n + eps)).  With S1 = sum |v|, S2 = sum v^2, n = M:
  s1:    a term carries its subtraction                                            ds1   = (depth + 1) u S1
  s2:    a term carries the subtraction twice and the product                      ds2   = (depth + 3) u S2
  d:     the division                                                              dd    = ds1 / n + u |d|
  mean:  the addition of the (exact) shift                                         dmean = dd + u |mean|
  m2:    = S2 - s1 d = sum (z - mean)^2 exactly; the product s1 d is off by |s1| dd + |d| ds1 + dd ds1, the product and the subtraction
         round once each (2 charged each); max(., 0) moves the value towards the reference, which is >= 0:
                                                    dm2   = ds2 + |s1| dd + |d| ds1 + dd ds1 + 2 u |s1 d| + 2 u m2
  a:     = m2 / n + eps, the division and the addition                             da    = dm2 / n + 3 u a
  rstd:  a -> a^-1/2 is monotone; sqrtf and the division are within 2 ulp = 4 u together:
                                                    drstd = (a - da)^-1/2 - rstd + 4 u (a - da)^-1/2       (infinite if da >= a)
  The shift makes S1, S2 of the size of the spread, not of the mean.  When row 0 is an outlier they are of the size of the outlier and
  the bound says so; da >= a would mean that the bound says nothing, and the tests assert that it does not happen for their inputs.
  This is the derivation of the issue; emulating the kernel's summation order in float32 on the CPU (test_clf_kernels_cpu.py) gives a
  worst error / bound of 0.76 (the mean of the sigma = 1e-3 channel: the single rounding of k + d, charged exactly once) and 0.15 to
  0.52 for the other three, the figures the MI355X gives as well; no count had to be changed.
  Running statistics, with the f32 values of eps and momentum and w = 1 - mom in float64 (the kernel's 1.f - mom rounds once):
  new = w old + mom x.  w old carries the rounding of w, the product and the addition (4 u charged); mom x the product and the addition
  (3 u), for the variance x = m2 / (n - 1) also the division (4 u); x itself is off by dmean, or by dm2 / (n - 1):
        drm = 4 u |w rm| + 3 u |mom mean| + mom dmean           drv = 4 u |w rv| + 4 u |mom x| + mom dm2 / (n - 1)
  num_batches_tracked is an integer: exact.

Apply (bn_apply; from the mean / rstd tensors GIVEN to the kernel): T = gamma ((z - mean) rstd) carries 3 roundings, the addition of
beta a fourth:                                               dy = 5 u |T| + u |beta|
  second branch: o += T2 + beta2 -- T and T2 pass 5 roundings, beta and beta2 two:   6 u (|T| + |T2|) + 3 u (|beta| + |beta2|)
  residual: o += res -- T passes 5, beta 2, res 1:                                   6 u |T| + 3 u |beta| + u |res|
  max(., 0) is 1-Lipschitz: the bound passes through the ReLU.

Backward (bn_bwd; from the GIVEN mean, rstd, gamma and a GIVEN y, so that no ReLU decision sits on a rounding).  g = dy, or
dpool[r / rows_per_batch] * pool_scale (one rounding: e0 = 1, else e0 = 0), masked by y > 0; xh = (z - mean) rstd:
  dbeta  = sum g:       (depth + e0) u sum |g|
  dgamma = sum g xh:    a term carries xh's two roundings and the product:     (depth + 3 + e0) u sum |g xh|
  dz = (gamma rstd) (g - dbeta inv_n - xh (dgamma inv_n)), inv_n = 1 / n rounded once.  t1 = dbeta / n passes inv_n, its product, the
  two subtractions, gamma rstd and the last product: 6 roundings; t2 = xh dgamma / n passes xh's two, inv_n and two products, one
  subtraction and the last two: 8; g passes the two subtractions and the last two: 4 + e0.  The computed dbeta / dgamma are within their
  own bounds of the reference's:
        ddz = |gamma rstd| (ddbeta / n + |xh| ddgamma / n + u ((5 + e0) |g| + 7 |t1| + 9 |t2|))
  g_out = g: exact in f32 for dy, one rounding for dpool.  With two branches both share dbeta; each has its own dgamma and dz.

BCE (bce; bce_sigmoid_kernel: p = 1 / (1 + expf(-z)), term = (y - 1) max(log1pf(-p), -100) - y max(logf(p), -100),
dlogit = (p - y) / max((1 - p) p, 1e-12) / B * (1 - p) * p).  As the BCE paragraph of step_kernels_common: p is within 6 u q of
q = sigmoid(z); logf(p) within 6 u + 4 u |log q|; log1pf(-p) within 6 u q / (1 - q) + u + 4 u |log(1 - q)| (for |z| <= 15 that term
is below 1.2 and the true error, about 2 u / (1 - q) + 4 u, three times smaller: the first-order form is safe there and only there, and no
clamp is active; the restatement asserts |z| <= 15).  A thread adds ceil(B / 256) terms, a 256-wide tree follows (8 levels), a term's
two monomials carry a product and the subtraction, the total the division by B:
        dloss = (sum born + (ceil(B / 256) + 8 + 3) u (sum |monomials| + sum born)) / B
  dlogit re-uses the SAME computed p and 1 - p in the quotient and in the products, so it is (p^ - y) / B with 6 roundings (the
  difference, (1 - p) p, two divisions, two products):                 ddlogit = (6 u q + 7 u |q - y|) / B

BatchNorm fold (bn_fold): s = gamma / sqrtf(var + eps) carries 3 roundings, w s a fourth: dw = 5 u |w s|; the bias beta - mean s:
mean s passes 5 roundings, beta one:  db = 6 u |mean s| + u |beta|.

Max-pool (maxpool_fwd / maxpool_bwd): plain loops over the windows and their in-bounds taps in (ky, kx) order with torch's rule --
the running maximum starts at -inf with the first in-bounds tap as its position, and a tap replaces it when `val > max or isnan(val)`:
the first maximum wins, the last NaN wins, a window of -inf keeps its first tap.  The forward only moves values: exact in any type.
The backward adds the dy of the windows whose position is the pixel, at most four:  cnt u sum |dy|  (0 for a single contribution)."""
import numpy as np
import torch
import torch.nn.functional as F

from step_kernels_common import INF, U32, half_ulp_bf16, out_bound, worst_ratio          # noqa: F401  (re-exported)

EPS_BN32 = float(np.float32(1e-5))          # what the kernels receive for eps = 1e-5 and momentum = 0.1
MOM32 = float(np.float32(0.1))

# (M, C, chunks or None where the issue's table leaves it open, why)
BN_PLANS = [(1, 4, 1, "one row, one active column quad"), (15, 72, None, "fewer than 16 rows"),
            (17, 72, None, "more than 16 rows, a tail tile of channels"), (65, 64, 2, "two chunks"), (663, 72, 11, "the older tests' shape"),
            (4100, 68, 65, "more than 64 chunks"), (4161, 8, 66, "more than 64 chunks"), (8200, 8, 129, "lane 0 adds three partials"),
            (8, 2048, 1, "the widest layer"), (130, 2048, 3, "the widest layer")]


def _cdiv(a, b):
    return -(-a // b)


def bn_plan(M, C):
    """csrc/clf_train.hip bn_chunks and the launchers -> (chunks, rows per chunk, depth of the reduction)"""
    ctiles = _cdiv(C, 64)
    chunks = max(1, min(1024 // ctiles, _cdiv(M, 64)))
    rpc = _cdiv(M, chunks)
    return chunks, rpc, _cdiv(rpc, 16) + 16 + _cdiv(chunks, 64) + 6


def _rsqrt_hi(a, da):
    lo = a - da
    return torch.where(lo > 0, lo.clamp_min(1e-300).rsqrt(), torch.full_like(a, INF))


# ------------------------------------------------------------------------------------------------------------- statistics
def bn_stats(z, rm=None, rv=None, eps=EPS_BN32, mom=MOM32):
    """z [M, C]; rm, rv [C] the running statistics BEFORE the call (or None); eps, mom the f32 values handed to the kernel
    -> dict(mean, dmean, rstd, drstd [, rm, drm, rv, drv]) in float64"""
    zd = z.double()
    M, C = zd.shape
    n, depth = float(M), bn_plan(M, C)[2]
    k = zd[0]
    v = zd - k
    S1, S2, s1 = v.abs().sum(0), (v * v).sum(0), v.sum(0)
    ds1, ds2 = (depth + 1) * U32 * S1, (depth + 3) * U32 * S2
    d = s1 / n
    mean = k + d
    dd = ds1 / n + U32 * d.abs()
    dmean = dd + U32 * mean.abs()
    m2 = ((zd - mean) ** 2).sum(0)
    dm2 = ds2 + s1.abs() * dd + d.abs() * ds1 + dd * ds1 + 2 * U32 * (s1 * d).abs() + 2 * U32 * m2
    a = m2 / n + eps
    da = dm2 / n + 3 * U32 * a
    rstd, hi_r = a.rsqrt(), _rsqrt_hi(a, da)
    out = dict(mean=mean, dmean=dmean, rstd=rstd, drstd=(hi_r - rstd) + 4 * U32 * hi_r)
    if rm is not None:
        w = 1.0 - mom
        A, Bm = w * rm.double(), mom * mean
        out.update(rm=A + Bm, drm=4 * U32 * A.abs() + 3 * U32 * Bm.abs() + mom * dmean)
        A, Bv = w * rv.double(), mom * m2 / (n - 1)
        out.update(rv=A + Bv, drv=4 * U32 * A.abs() + 4 * U32 * Bv.abs() + mom * dm2 / (n - 1))
    return out


def stats_input(M, C, seed, device="cpu"):
    """f32 [M, C] whose channels are N(c / C, (0.1 + c / C)^2) but for: 0 -- mean = 1000 sigma; 1 -- row 0 an outlier of 1000;
    C - 2 -- constant; C - 1 -- sigma = 1e-3 around 5 (C = 4: nothing else)"""
    g = torch.Generator().manual_seed(seed)
    ch = torch.arange(C, dtype=torch.float32) / C
    z = torch.randn((M, C), generator=g) * (0.1 + ch) + ch
    z[:, 0] = 1000.0 + torch.randn((M,), generator=g)
    z[:, 1] = torch.randn((M,), generator=g)
    z[0, 1] = 1000.0
    z[:, C - 2] = 7.25
    z[:, C - 1] = 5.0 + 1e-3 * torch.randn((M,), generator=g)
    return z.to(device)


# ------------------------------------------------------------------------------------------------------------- apply
def _bn_T(z, mean, rstd, gamma):
    return gamma.double() * ((z.double() - mean.double()) * rstd.double())


def bn_apply(z, mean, rstd, gamma, beta, relu, second=None, residual=None):
    """second = (z2, mean2, rstd2, gamma2, beta2) -> (y float64, the f32-level bound)"""
    T, b = _bn_T(z, mean, rstd, gamma), beta.double()
    if second is not None:
        T2, b2 = _bn_T(*second[:4]), second[4].double()
        y = T + b + (T2 + b2)
        bound = 6 * U32 * (T.abs() + T2.abs()) + 3 * U32 * (b.abs() + b2.abs())
    elif residual is not None:
        r = residual.double()
        y = T + b + r
        bound = 6 * U32 * T.abs() + 3 * U32 * b.abs() + U32 * r.abs()
    else:
        y = T + b
        bound = 5 * U32 * T.abs() + U32 * b.abs()
    return (y.clamp_min(0) if relu else y), bound


# ------------------------------------------------------------------------------------------------------------- backward
BWD_MUTANTS = ("inv_m1", "mask_ge", "dpool_mod", "mean_shared", "drop_chunk")


def bn_bwd(branches, dy=None, dpool=None, rows_per_batch=0, pool_scale=1.0, y=None, mutant=None):
    """branches: [(z, mean, rstd, gamma)], one or two; the gradient is dy [M, C] or dpool [M / rows_per_batch, C] * pool_scale (its f32
    value) spread over rows_per_batch rows each; y [M, C]: the saved output whose sign masks the gradient (or None)
    -> dict(g, dg, dbeta, ddbeta, dgamma [..], ddgamma [..], dz [..], ddz [..]) in float64.
    mutant: one of BWD_MUTANTS, the defects of test_clf_kernels_cpu.py"""
    assert mutant is None or mutant in BWD_MUTANTS
    z0 = branches[0][0]
    M, C = z0.shape
    n = float(M)
    chunks, rpc, depth = bn_plan(M, C)
    rows = torch.arange(M, device=z0.device)
    if dy is not None:
        g, e0 = dy.double(), 0
    else:
        idx = rows % rows_per_batch % dpool.shape[0] if mutant == "dpool_mod" else rows // rows_per_batch
        g, e0 = dpool.double()[idx] * pool_scale, 1
    if y is not None:
        g = g * ((y.double() >= 0) if mutant == "mask_ge" else (y.double() > 0))
    keep = torch.ones((M, 1), dtype=torch.float64, device=z0.device)
    if mutant == "drop_chunk":
        keep[(chunks - 1) * rpc:] = 0
    dbeta, ddbeta = (g * keep).sum(0), (depth + e0) * U32 * g.abs().sum(0)
    out = dict(g=g, dg=e0 * U32 * g.abs(), dbeta=dbeta, ddbeta=ddbeta, dgamma=[], ddgamma=[], dz=[], ddz=[])
    for b, (z, mean, rstd, gamma) in enumerate(branches):
        mu = (branches[0][1] if (mutant == "mean_shared" and b == 1) else mean).double()
        rs, gm = rstd.double(), gamma.double()
        xh = (z.double() - mu) * rs
        dgamma, ddgamma = (g * xh * keep).sum(0), (depth + 3 + e0) * U32 * (g * xh).abs().sum(0)
        nn = n - 1 if mutant == "inv_m1" else n
        t1, t2 = dbeta / nn, xh * dgamma / nn
        dz = gm * rs * (g - t1 - t2)
        ddz = (gm * rs).abs() * (ddbeta / n + xh.abs() * ddgamma / n + U32 * ((5 + e0) * g.abs() + 7 * t1.abs() + 9 * t2.abs()))
        out["dgamma"].append(dgamma), out["ddgamma"].append(ddgamma), out["dz"].append(dz), out["ddz"].append(ddz)
    return out


def bwd_case(M, C, rows_per_batch, two, seed, device="cpu", dtype=torch.float32):
    """what the GPU file feeds the backward: random z, given statistics near the true ones, a synthesised y with exact zeros and
    negative values"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(shape, generator=g)
    z, z2 = (rn(M, C) * 1.5 + 0.3).to(dtype), (rn(M, C) * 0.7 - 0.2).to(dtype)
    y = rn(M, C)
    y[torch.rand((M, C), generator=g) < 0.2] = 0.0
    br = [(z, z.float().mean(0) + 0.01 * rn(C), 1.0 / (z.float().std(0, unbiased=False) + 0.1) if M > 1 else torch.ones(C), rn(C).abs() + 0.5)]
    if two:
        br.append((z2, z2.float().mean(0) - 0.01 * rn(C), 1.0 / (z2.float().std(0, unbiased=False) + 0.1) if M > 1 else torch.ones(C), rn(C) - 0.2))
    if rows_per_batch:
        src = dict(dpool=rn(M // rows_per_batch, C), rows_per_batch=rows_per_batch, pool_scale=float(np.float32(1.0 / rows_per_batch)))
    else:
        src = dict(dy=rn(M, C).to(dtype))
    mv = lambda t: t.to(device) if torch.is_tensor(t) else t
    return [tuple(mv(t) for t in b) for b in br], {k: mv(v) for k, v in src.items()}, y.to(dtype).to(device)


def bwd_exact_inputs(M, C, seed, device="cpu"):
    """z, dy integers in [-8, 8], mean an integer per channel in [-4, 4], rstd = 1/2, y in {-1, 0, 1} (a third of each): xh is a
    half-integer below 7, g xh a half-integer below 56, a sum of up to 2^14 of them a multiple of 1/2 below 2^20: exact in f32 in any
    order (and every input is exact in bf16)"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda shape, m: torch.randint(-m, m + 1, shape, generator=g).float()
    return dict(z=ri((M, C), 8).to(device), dy=ri((M, C), 8).to(device), mean=ri((C,), 4).to(device),
                rstd=torch.full((C,), 0.5, device=device), y=ri((M, C), 1).to(device), z2=ri((M, C), 8).to(device),
                mean2=ri((C,), 4).to(device))


# ------------------------------------------------------------------------------------------------------------- BCE
def bce(logit, label, drop_from=None):
    """-> dict(loss, dloss (0-dim); dlogit, ddlogit [B]) in float64.  drop_from = k: the CPU file's mutant, the elements >= k are left
    out of the loss's sum"""
    z, t = logit.double(), label.double()
    B = z.numel()
    assert float(z.abs().max()) <= 15, "the first-order bound of log(1 - q) and the inactive clamps need |z| <= 15"
    q = torch.sigmoid(z)
    lq, l1q = F.logsigmoid(z), F.logsigmoid(-z)
    m1, m2 = (t - 1) * l1q, -t * lq
    born = (1 - t).abs() * (6 * U32 * q / (1 - q) + U32 + 4 * U32 * l1q.abs()) + t.abs() * (6 * U32 + 4 * U32 * lq.abs())
    keep = torch.ones_like(z)
    if drop_from is not None:
        keep[drop_from:] = 0
    depth = _cdiv(B, 256) + 8
    loss = ((m1 + m2) * keep).sum() / B
    dloss = (born.sum() + (depth + 3) * U32 * ((m1.abs() + m2.abs()).sum() + born.sum())) / B
    return dict(loss=loss, dloss=dloss, dlogit=(q - t) / B, ddlogit=(6 * U32 * q + 7 * U32 * (q - t).abs()) / B)


# ------------------------------------------------------------------------------------------------------------- fold
def bn_fold(w, gamma, beta, mean, var, eps):
    """w [Co, K] -> (w' float64 [Co, K], its f32-level bound, bias [Co], its bound)"""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    wf, ms = w.double() * s[:, None], mean.double() * s
    return wf, 5 * U32 * wf.abs(), beta.double() - ms, 6 * U32 * ms.abs() + U32 * beta.double().abs()


# ------------------------------------------------------------------------------------------------------------- max-pool
def _windows(H, W):
    """(oy, ox, [(tap, iy, ix)]) of MaxPool2d(3, 2, 1): the in-bounds taps in (ky, kx) order"""
    for oy in range((H - 1) // 2 + 1):
        for ox in range((W - 1) // 2 + 1):
            yield oy, ox, [(ky * 3 + kx, oy * 2 - 1 + ky, ox * 2 - 1 + kx) for ky in range(3) for kx in range(3)
                           if 0 <= oy * 2 - 1 + ky < H and 0 <= ox * 2 - 1 + kx < W]


def _window_max(xb, taps):
    """xb [H, W, C] -> (max [C], position [C] as an index into taps)"""
    C = xb.shape[-1]
    m = torch.full((C,), -INF, dtype=xb.dtype, device=xb.device)
    pos = torch.zeros((C,), dtype=torch.long, device=xb.device)
    for i, (_, iy, ix) in enumerate(taps):
        v = xb[iy, ix]
        take = (v > m) | torch.isnan(v)
        m, pos = torch.where(take, v, m), torch.where(take, torch.full_like(pos, i), pos)
    return m, pos


def maxpool_fwd(x):
    """x [B, H, W, C] -> [B, Ho, Wo, C] float64"""
    xd = x.double()
    B, H, W, C = xd.shape
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float64, device=x.device)
    for b in range(B):
        for oy, ox, taps in _windows(H, W):
            y[b, oy, ox] = _window_max(xd[b], taps)[0]
    return y


def maxpool_bwd(dy, x):
    """-> (dx float64 [B, H, W, C], the f32-level bound, dx added in f32 in window order (oy, ox): what an f32 gather gives bit for bit)"""
    xd, d = x.double(), dy.double()
    B, H, W, C = xd.shape
    dx, S, cnt = torch.zeros_like(xd), torch.zeros_like(xd), torch.zeros_like(xd)
    dx32 = torch.zeros(xd.shape, dtype=torch.float32, device=x.device)
    for b in range(B):
        for oy, ox, taps in _windows(H, W):
            _, pos = _window_max(xd[b], taps)
            for i, (_, iy, ix) in enumerate(taps):
                hit = pos == i
                dx[b, iy, ix] += torch.where(hit, d[b, oy, ox], torch.zeros_like(d[b, oy, ox]))
                dx32[b, iy, ix] += torch.where(hit, dy[b, oy, ox].float(), torch.zeros((C,), device=x.device))
                S[b, iy, ix] += torch.where(hit, d[b, oy, ox].abs(), torch.zeros_like(d[b, oy, ox]))
                cnt[b, iy, ix] += hit.double()
    return dx, torch.where(cnt > 1, cnt * U32 * S, torch.zeros_like(S)), dx32


POOL_SHAPES = [(2, 1, 1, 4), (1, 1, 9, 8), (1, 2, 2, 4), (2, 13, 18, 8), (1, 8, 8, 12)]          # (B, H, W, C)


def pool_input(B, H, W, C, seed):
    """f32 [B, H, W, C] with both signs, planted ties, (H, W >= 5) one window of -inf in channel 1 and one NaN in channel 2 whose
    windows also hold larger finite values; H, W < 5: the -inf window and the NaN are image 0's whole channel 1 and pixel (0, 0, 2)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, C), generator=g)
    x[:, :3, :3, 0] = 0.75 if H > 1 else -0.75                 # ties: the first maximum in scan order takes the gradient
    x[:, H // 2:, W // 2:, 3] = -1.5                           # ties between negative values
    if H >= 5 and W >= 5:
        x[0, 1:4, 1:4, 1] = -INF                               # the window of output (1, 1), all of it
        x[0, 2, 3, 2] = float("nan")
        x[0, 2, 4, 2] = 50.0                                   # larger than the NaN's neighbours: must not hide it
    else:
        x[0, :, :, 1] = -INF
        x[0, 0, 0, 2] = float("nan")
        if W > 1:
            x[0, 0, 1, 2] = 50.0
    return x


# ------------------------------------------------------------------------------------------------------------- im2col
def im2col(x, KH, KW, stride, pad):
    """x [B, C, H, W] -> rows [B * Ho * Wo, C * KH * KW], K order (c, ky, kx): F.unfold, a pure move"""
    return F.unfold(x, kernel_size=(KH, KW), padding=pad, stride=stride).transpose(1, 2).reshape(-1, x.shape[1] * KH * KW)
