"""tests/clf_kernels_common.py checked without a GPU: (1) every float64 restatement equals something independent of it (F.batch_norm,
F.max_pool2d, F.binary_cross_entropy, F.unfold, autograd); (2) the statistics bound holds for a float32 emulation of the kernel's own
summation order, and every bound can fail: a result with a named defect, rounded to the kernel's output type, exceeds it at a shape of
the GPU file's list; (3) the inputs of the GPU file's exact test are exact; (4) the plan mirror gives what the library computes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clf_kernels_common as ck

EPS, MOM = ck.EPS_BN32, ck.MOM32
PLAN_IDS = [f"{M}x{C}" for M, C, _, _ in ck.BN_PLANS]


def _randn(shape, seed, dtype=torch.float64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _close(a, b, scale=None):
    """float64 against float64 in another order"""
    s = (b.abs().max() if scale is None else scale) + 1e-300
    return float((a - b).abs().max() / s) <= 1e-11


# ------------------------------------------------------------------------------------------------------------- (4) plan mirror
def test_plan_mirror_is_the_library():
    from unmore_amd import _lib
    lib = _lib.lib()
    for M, C, chunks, _ in ck.BN_PLANS:
        got, rpc, depth = ck.bn_plan(M, C)
        assert chunks is None or got == chunks, (M, C, got)
        assert lib.umr_bn_train_workspace(M, C) == got * 3 * C * 4, (M, C)
        assert got * rpc >= M > (got - 1) * rpc                           # every chunk but possibly the last is full, none is empty
        assert depth == -(-rpc // 16) + 16 + -(-got // 64) + 6
    assert ck.bn_plan(4161, 8)[0] > 64 and ck.bn_plan(8200, 8)[0] > 128 and ck.bn_plan(4096, 8)[0] == 64


# ------------------------------------------------------------------------------------------------------------- (1) restatements
@pytest.mark.parametrize("M,C", [(2, 4), (17, 72), (65, 64)])
def test_bn_restatements_match_batch_norm_and_autograd(M, C):
    z, z2, res = _randn((M, C), 1) * 1.5 + 0.3, _randn((M, C), 2) * 0.7 - 0.2, _randn((M, C), 3)
    g, b, g2, b2 = _randn((C,), 4), _randn((C,), 5), _randn((C,), 6), _randn((C,), 7)
    rm, rv = _randn((C,), 8), _randn((C,), 9).abs() + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    F.batch_norm(z, rm_t, rv_t, None, None, True, MOM, EPS)
    s, s2 = ck.bn_stats(z, rm, rv), ck.bn_stats(z2)
    assert _close(s["mean"], z.mean(0)) and _close(s["rstd"], (z.var(0, unbiased=False) + EPS).rsqrt())
    assert _close(s["rm"], rm_t) and _close(s["rv"], rv_t)
    for k in ("dmean", "drstd", "drm", "drv"):
        assert bool((s[k] > 0).all()) and bool(torch.isfinite(s[k]).all())
    B = M // 1 if M % 5 else M // 5
    for two in (False, True):
        for relu in (False, True):
            for pooled in (False, True):
                zt, z2t, gt, bt, g2t, b2t = (t.clone().requires_grad_(True) for t in (z, z2, g, b, g2, b2))
                o = F.batch_norm(zt, None, None, gt, bt, True, MOM, EPS)
                o = o + (F.batch_norm(z2t, None, None, g2t, b2t, True, MOM, EPS) if two else res)
                y = o.clamp_min(0) if relu else o
                second = (z2, s2["mean"], s2["rstd"], g2, b2) if two else None
                yr, by = ck.bn_apply(z, s["mean"], s["rstd"], g, b, relu, second=second, residual=None if two else res)
                assert _close(yr, y.detach()) and bool((by >= 0).all())
                rpb = M // B
                if pooled:
                    dpool = _randn((B, C), 10)
                    (y.view(B, rpb, C).mean(1) * dpool).sum().backward()
                    src = dict(dpool=dpool, rows_per_batch=rpb, pool_scale=1.0 / rpb)
                    gref = (dpool / rpb).repeat_interleave(rpb, 0)
                else:
                    dy = _randn((M, C), 11)
                    (y * dy).sum().backward()
                    src, gref = dict(dy=dy), dy
                br = [(z, s["mean"], s["rstd"], g)] + ([(z2, s2["mean"], s2["rstd"], g2)] if two else [])
                w = ck.bn_bwd(br, y=y.detach() if relu else None, **src)
                assert _close(w["g"], gref * (y.detach() > 0) if relu else gref)
                assert _close(w["dz"][0], zt.grad) and _close(w["dgamma"][0], gt.grad) and _close(w["dbeta"], bt.grad)
                if two:
                    assert _close(w["dz"][1], z2t.grad) and _close(w["dgamma"][1], g2t.grad) and _close(w["dbeta"], b2t.grad)
    # the single form without the other operand
    yr, _ = ck.bn_apply(z, s["mean"], s["rstd"], g, b, True)
    assert _close(yr, F.batch_norm(z, None, None, g, b, True, MOM, EPS).clamp_min(0))


@pytest.mark.parametrize("B,H,W,C", ck.POOL_SHAPES)
def test_maxpool_restatement_matches_torch(B, H, W, C):
    """torch returns the NaN in the forward, routes its window's gradient to it, and routes the gradient of a window of -inf to the
    window's first in-bounds pixel: the restatement's rule"""
    x = ck.pool_input(B, H, W, C, 1).double()
    assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and bool((x < 0).any())
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt = F.max_pool2d(xt, 3, 2, 1)
    y = ck.maxpool_fwd(x)
    want = yt.detach().permute(0, 2, 3, 1)
    assert bool(torch.isnan(want).any()) and bool((want == -ck.INF).any())
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and torch.equal(torch.nan_to_num(y, 123.0), torch.nan_to_num(want, 123.0))
    dy = _randn(tuple(y.shape), 2)
    yt.backward(dy.permute(0, 3, 1, 2))
    dx, bound, dx32 = ck.maxpool_bwd(dy, x)
    assert _close(dx, xt.grad.permute(0, 2, 3, 1)) and bool((bound >= 0).all())
    assert float((dx32.double() - dx).abs().max()) < 1e-5                   # f32 sums of at most four f32-rounded values
    assert float(dx.sum()) == pytest.approx(float(dy.sum()), rel=1e-12)     # every window gives its gradient to exactly one pixel


def test_bce_restatement_matches_torch():
    for B in (1, 257, 1000):
        z = (torch.rand(B, generator=torch.Generator().manual_seed(B), dtype=torch.float64) * 2 - 1) * 15
        t = (torch.arange(B) % 2).double()
        zt = z.clone().requires_grad_(True)
        loss = F.binary_cross_entropy(torch.sigmoid(zt), t)
        loss.backward()
        r = ck.bce(z, t)
        assert abs(float(r["loss"] - loss.detach())) <= 1e-9 * float(loss.detach())          # torch forms log(1 - sigmoid) by a subtraction
        assert _close(r["dlogit"], zt.grad) and float(r["dloss"]) > 0 and bool((r["ddlogit"] > 0).all())
    with pytest.raises(AssertionError):
        ck.bce(torch.tensor([15.5]), torch.tensor([0.0]))


@pytest.mark.parametrize("B,C,H,W,KH,KW,stride,pad", [(2, 3, 9, 11, 7, 7, 2, 3), (1, 3, 1, 1, 7, 7, 2, 3), (2, 2, 6, 7, 3, 5, 1, 0),
                                                      (1, 5, 8, 9, 3, 3, 2, 1)])
def test_im2col_reference_is_the_plain_loop(B, C, H, W, KH, KW, stride, pad):
    x = _randn((B, C, H, W), 1)
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    want = torch.zeros((B, Ho, Wo, C, KH, KW), dtype=torch.float64)
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(KH):
                for kx in range(KW):
                    iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
                    if 0 <= iy < H and 0 <= ix < W:
                        want[:, oy, ox, :, ky, kx] = x[:, :, iy, ix]
    assert torch.equal(ck.im2col(x, KH, KW, stride, pad), want.reshape(B * Ho * Wo, C * KH * KW))


def test_fold_restatement_matches_eval_batch_norm():
    Co, K = 5, 27
    w, x = _randn((Co, K), 1), _randn((9, K), 2)
    g, b, m, v = _randn((Co,), 3), _randn((Co,), 4), _randn((Co,), 5), _randn((Co,), 6).abs() + 0.3
    wf, dw, bf, db = ck.bn_fold(w, g, b, m, v, EPS)
    assert _close(x @ wf.t() + bf, F.batch_norm(x @ w.t(), m, v, g, b, False, MOM, EPS))
    assert bool((dw > 0).all()) and bool((db > 0).all())
    one, zero = torch.ones(Co, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64)
    wf, _, bf, _ = ck.bn_fold(w, one, zero, zero, one, 0.0)
    assert torch.equal(wf, w) and torch.equal(bf, zero)


# ------------------------------------------------------------------------------------------------------------- (2) statistics: emulation
def emulate_stats(z, rm, rv, shift=True, drop_last_row=False, drop_chunks_ge64=False, biased=False):
    """bn_stats_partial_kernel + bn_stats_final_kernel in numpy float32, addition by addition in the kernels' order (no fused
    multiply-add).  z [M, C] float32.  The keyword arguments are the mutants.  -> (mean, rstd, rm', rv') float32"""
    f = np.float32
    M, C = z.shape
    chunks, rpc, _ = ck.bn_plan(M, C)
    iters = -(-rpc // 16)
    k = z[0] if shift else np.zeros(C, f)
    j = np.arange(iters * 16).reshape(1, iters, 16)                         # row of the chunk = iteration * 16 + row lane
    idx = np.arange(chunks).reshape(-1, 1, 1) * rpc + j
    valid = (j < rpc) & (idx < M)
    if drop_last_row:
        valid &= idx != M - 1
    v = np.where(valid[..., None], z[np.minimum(idx, M - 1)] - k, f(0)).astype(f)     # [chunks, iters, 16, C]
    a1, a2 = np.zeros((chunks, 16, C), f), np.zeros((chunks, 16, C), f)
    for it in range(iters):
        a1 = a1 + v[:, it]
        a2 = a2 + v[:, it] * v[:, it]
    p1, p2 = np.zeros((chunks, C), f), np.zeros((chunks, C), f)
    for rl in range(16):
        p1, p2 = p1 + a1[:, rl], p2 + a2[:, rl]
    l1, l2 = np.zeros((64, C), f), np.zeros((64, C), f)
    for c in range(chunks if not drop_chunks_ge64 else min(chunks, 64)):
        l1[c % 64] = l1[c % 64] + p1[c]
        l2[c % 64] = l2[c % 64] + p2[c]
    for o in (32, 16, 8, 4, 2, 1):
        l1, l2 = l1 + l1[np.arange(64) ^ o], l2 + l2[np.arange(64) ^ o]
    s1, s2, n = l1[0], l2[0], f(M)
    assert s1.dtype == f and v.dtype == f and p2.dtype == f
    d = s1 / n
    m2 = np.maximum(s2 - s1 * d, f(0))
    mu = k + d
    rstd = f(1) / np.sqrt(m2 / n + f(EPS))
    w = f(1) - f(MOM)
    rm_new = w * rm + f(MOM) * mu
    rv_new = w * rv + f(MOM) * (m2 / (n if biased else n - f(1)))
    assert rstd.dtype == f and rv_new.dtype == f
    return mu, rstd, rm_new, rv_new


def _stats_ratios(z, got, rm, rv):
    """worst error / bound per quantity of an emulated (or mutated) result against bn_stats of the same z"""
    r = ck.bn_stats(z, rm, rv)
    assert bool(torch.isfinite(r["drstd"]).all()), "da >= a: the bound says nothing for this input"
    out = {}
    for name, val, bound in (("mean", got[0], "dmean"), ("rstd", got[1], "drstd"), ("rm", got[2], "drm"), ("rv", got[3], "drv")):
        out[name] = ck.worst_ratio(torch.from_numpy(np.asarray(val, np.float32)), r[name], r[bound])[0]
    return out


def _stats_case(M, C, bf16):
    z = ck.stats_input(M, C, M * 7 + C)
    if bf16:
        z = z.bfloat16().float()
    g = torch.Generator().manual_seed(M + C)
    return z, torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g).abs() + 0.5


STAT_SHAPES = [(M, C) for M, C, _, _ in ck.BN_PLANS if M > 1]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_statistics_bound_holds_for_the_kernels_summation_order(bf16):
    worst = {}
    for M, C in STAT_SHAPES + [(2, 8)]:
        z, rm, rv = _stats_case(M, C, bf16)
        ratios = _stats_ratios(z, emulate_stats(z.numpy(), rm.numpy(), rv.numpy()), rm, rv)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("emulated statistics, worst error / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert max(worst.values()) > 0.01, "a bound a hundred times above the emulation's error would hide a defect"
    # M = 1: v = 0, the mean is the row, rstd = eps^-1/2 to the rounding of rsqrt
    z = ck.stats_input(1, 4, 1)
    r = ck.bn_stats(z)
    assert torch.equal(r["mean"], z[0].double()) and bool(torch.isfinite(r["drstd"]).all())


@pytest.mark.parametrize("name,kw,shapes", [
    ("no shift", dict(shift=False), [(663, 72)]),
    ("biased running variance", dict(biased=True), [(15, 72), (663, 72)]),
    ("last row of the last chunk dropped", dict(drop_last_row=True), [(17, 72), (663, 72), (130, 2048)]),
    ("chunks >= 64 dropped", dict(drop_chunks_ge64=True), [(4100, 68), (4161, 8), (8200, 8)])])
def test_statistics_mutants_exceed_the_bound(name, kw, shapes):
    for M, C in shapes:
        z, rm, rv = _stats_case(M, C, False)
        ratios = _stats_ratios(z, emulate_stats(z.numpy(), rm.numpy(), rv.numpy(), **kw), rm, rv)
        print(f"{name} at {M}x{C}: worst error / bound", {k: round(v, 3) for k, v in ratios.items()})
        assert max(ratios.values()) > 1.0, (name, M, C, ratios)


# ------------------------------------------------------------------------------------------------------------- (2) backward, BCE: mutants
def _bwd_ratios(ref, got, dtype):
    out = {"g_out": ck.worst_ratio(got["g"].to(dtype), ref["g"], ck.out_bound(ref["g"], ref["dg"], dtype))[0],
           "dbeta": ck.worst_ratio(got["dbeta"].float(), ref["dbeta"], ref["ddbeta"])[0]}
    for b in range(len(ref["dz"])):
        out[f"dgamma{b}"] = ck.worst_ratio(got["dgamma"][b].float(), ref["dgamma"][b], ref["ddgamma"][b])[0]
        out[f"dz{b}"] = ck.worst_ratio(got["dz"][b].to(dtype), ref["dz"][b], ck.out_bound(ref["dz"][b], ref["ddz"][b], dtype))[0]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mutant,M,C,rpb,two", [("inv_m1", 663, 72, 0, False), ("mask_ge", 65, 64, 0, False), ("dpool_mod", 65, 64, 5, False),
                                                ("mean_shared", 15, 72, 0, True), ("drop_chunk", 4161, 8, 0, False),
                                                ("drop_chunk", 130, 2048, 1, True)])
def test_backward_mutants_exceed_the_bound(mutant, M, C, rpb, two, dtype):
    br, src, y = ck.bwd_case(M, C, rpb, two, 5, dtype=dtype)
    ref, bad = ck.bn_bwd(br, y=y, **src), ck.bn_bwd(br, y=y, mutant=mutant, **src)
    clean = _bwd_ratios(ref, ref, dtype)
    assert max(clean.values()) <= 1.0, clean                  # the reference rounded to the output type is inside its own bound
    ratios = _bwd_ratios(ref, bad, dtype)
    print(f"{mutant} at {M}x{C}: worst error / bound", {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) > 1.0, (mutant, ratios)


def test_bce_mutant_exceeds_the_bound():
    """at |z| <= 15 the bound is dominated by what f32 loses in 1 - sigmoid(z) near z = 15 (about 1 / B per such element with label 0):
    744 dropped elements exceed it, a single one need not; at |z| <= 4 a single dropped element does"""
    for B, zmax in ((1000, 15.0), (257, 4.0)):
        z = (torch.rand(B, generator=torch.Generator().manual_seed(B)) * 2 - 1) * zmax
        t = (torch.arange(B) % 2).float()
        r, bad = ck.bce(z, t), ck.bce(z, t, drop_from=256)
        print(f"BCE B={B} |z|<={zmax}: bound {float(r['dloss']):.3e}, mutant off by {abs(float(bad['loss'] - r['loss'])):.3e}")
        assert abs(float(bad["loss"].float().double() - r["loss"])) > float(r["dloss"]), (B, float(r["dloss"]))
        assert abs(float(r["loss"].float().double() - r["loss"])) <= float(r["dloss"])


# ------------------------------------------------------------------------------------------------------------- (3) exact inputs
@pytest.mark.parametrize("M,C", [(M, C) for M, C, _, _ in ck.BN_PLANS], ids=PLAN_IDS)
def test_exact_backward_inputs_are_exact(M, C):
    """the two sums in float32, in reversed row order and by halves, give float64's bits; every input survives bf16"""
    e = ck.bwd_exact_inputs(M, C, M + C)
    g = e["dy"] * (e["y"] > 0)
    assert bool((e["y"] == 0).any()) or M * C < 16
    for z, mean in ((e["z"], e["mean"]), (e["z2"], e["mean2"])):
        t = g * ((z - mean) * e["rstd"])
        assert t.dtype == torch.float32
        want = t.double().sum(0)
        assert torch.equal(t.flip(0).sum(0).double(), want) and torch.equal((t[: M // 2].sum(0) + t[M // 2:].sum(0)).double(), want)
        assert torch.equal(z.bfloat16().float(), z)
    assert torch.equal(g.flip(0).sum(0).double(), g.double().sum(0))
    assert all(torch.equal(e[k].bfloat16().float(), e[k]) for k in ("dy", "y"))
    r = ck.bn_bwd([(e["z"], e["mean"], e["rstd"], torch.ones(C))], dy=e["dy"], y=e["y"])
    assert torch.equal(r["dbeta"], g.double().sum(0))
