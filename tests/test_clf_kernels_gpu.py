"""The existence classifier's hand-written kernels (csrc/clf_train.hip, csrc/classifier.hip), each called through its ops wrapper and
compared with the float64 restatement of tests/clf_kernels_common.py (itself checked against F.batch_norm / F.max_pool2d /
F.binary_cross_entropy / F.unfold and autograd in tests/test_clf_kernels_cpu.py).

 bounded: the reference is float64 on exactly the tensors the kernel is given; every element must obey |kernel - ref| <= bound, the bound
          being a function of clf_kernels_common built from reference quantities only (its docstring has the derivations).
          `worst error / bound` is printed for every kernel and type.
 exact:   pure moves (max-pool forward, im2col, the stride-2 scatter) must equal the reference bit for bit in either type, and the
          backward's two column sums must equal float64 for integer inputs at every launch plan of the list.
No tolerance below is a number of this file."""
import pytest
import torch
import torch.nn.functional as F

import clf_kernels_common as ck

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
PLANS = [(M, C) for M, C, _, _ in ck.BN_PLANS]
PLAN_IDS = [f"{M}x{C}" for M, C in PLANS]


def _ops():
    from unmore_amd import ops
    return ops


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def _randn(shape, seed, dtype=torch.float32, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale + shift).to(dtype)


def _nan(shape):
    return torch.full(shape, float("nan"), device=DEV)


def _check(label, out, ref, delta, tag=None):
    """every element of `out` within the bound that belongs to its type; prints worst error / bound"""
    ratio, bad = ck.worst_ratio(out, ref, ck.out_bound(ref, delta, out.dtype))
    print(f"worst error / bound  {label} [{tag or _name(out.dtype)}]: {ratio:.4f}")
    assert bad == 0, f"{label}: {bad} of {out.numel()} elements over their bound, worst error / bound = {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------------------------------------------------- plan list
def test_plan_list_reaches_the_plans_it_names():
    for M, C, chunks, _ in ck.BN_PLANS:
        assert chunks is None or ck.bn_plan(M, C)[0] == chunks
    assert ck.bn_plan(15, 72)[:2] == (1, 15) and ck.bn_plan(17, 72)[:2] == (1, 17)          # below / above the 16 row lanes
    assert sum(ck.bn_plan(M, C)[0] > 64 for M, C in PLANS) == 3 and ck.bn_plan(8200, 8)[0] > 128


# ------------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,C", PLANS, ids=PLAN_IDS)
def test_bn_statistics_bounded(M, C, dtype):
    ops = _ops()
    z = ck.stats_input(M, C, M * 7 + C, DEV).to(dtype)
    rm, rv = _randn((C,), 1, scale=0.1), _randn((C,), 2).abs() + 0.5
    tag = f"{M}x{C} {_name(dtype)}"
    if M == 1:
        with pytest.raises(RuntimeError, match="more than one value"):
            ops.bn_train_stats(z, rm.clone(), rv.clone(), None)
        mean, rstd = ops.bn_train_stats(z)
        r = ck.bn_stats(z)
    else:
        rm_d, rv_d, nbt = rm.clone(), rv.clone(), torch.full((), 41, dtype=torch.int64, device=DEV)
        mean, rstd = ops.bn_train_stats(z, rm_d, rv_d, nbt)           # eps = 1e-5, momentum = 0.1: the kernel gets their f32 values
        r = ck.bn_stats(z, rm, rv)
        _check("bn_stats running_mean", rm_d, r["rm"], r["drm"], tag)
        _check("bn_stats running_var", rv_d, r["rv"], r["drv"], tag)
        assert int(nbt) == 42
    assert bool(torch.isfinite(r["drstd"]).all()), "da >= a for a channel: the reference's bound says nothing about it"
    _check("bn_stats mean", mean, r["mean"], r["dmean"], tag)
    _check("bn_stats rstd", rstd, r["rstd"], r["drstd"], tag)


# ------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["single", "second", "residual"])
@pytest.mark.parametrize("M,C", [(17, 72), (663, 72)])
def test_bn_apply_bounded(M, C, form, dtype):
    ops = _ops()
    z, z2 = _randn((M, C), 1, dtype, 1.5, 0.3), _randn((M, C), 2, dtype, 2.0, 1.0)
    g, b, g2, b2 = _randn((C,), 3, shift=0.2), _randn((C,), 4), _randn((C,), 5, shift=-0.2), _randn((C,), 6)
    (mean, rstd), (mean2, rstd2) = ops.bn_train_stats(z), ops.bn_train_stats(z2)
    second = (z2, mean2, rstd2, g2, b2) if form == "second" else None
    res = z2 if form == "residual" else None
    for relu in (True, False):
        y = ops.bn_train_apply(z, mean, rstd, g, b, relu=relu, second=second, residual=res)
        ref, bound = ck.bn_apply(z, mean, rstd, g, b, relu, second=second, residual=res)
        _check(f"bn_apply {form} relu={int(relu)} {M}x{C}", y, ref, bound)
        if relu:
            assert bool((y >= 0).all()) and bool((y == 0).any())


# ------------------------------------------------------------------------------------------------------------- backward
def _run_bwd(br, src, y, want_g):
    C = br[0][0].shape[1]
    outs = [(_nan((C,)), _nan((C,))) for _ in br]
    got = _ops().bn_train_bwd([b + o for b, o in zip(br, outs)], y=y, want_g=want_g, **src)
    dzs, g = got if want_g else (got, None)
    return dict(dz=dzs, g=g, dgamma=[o[0] for o in outs], dbeta=[o[1] for o in outs])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("M,C", [(15, 72), (65, 64), (663, 72), (4161, 8), (130, 2048)])
def test_bn_backward_bounded(M, C, two, dtype):
    for rpb in (0, 1, 5, M):                # 0: the gradient is dy; else dpool over rpb rows each
        if rpb and M % rpb:
            continue
        br, src, y = ck.bwd_case(M, C, rpb, two, 100 + rpb, DEV, dtype)
        got = _run_bwd(br, src, y, want_g=True)
        ref = ck.bn_bwd(br, y=y, **src)
        tag = f"{'dpool/%d' % rpb if rpb else 'dy'} {M}x{C} {'two' if two else 'one'}"
        assert bool((y == 0).any()) and bool((y < 0).any())
        _check(f"bn_bwd g_out {tag}", got["g"], ref["g"], ref["dg"])
        for b in range(len(br)):
            _check(f"bn_bwd dbeta{b} {tag}", got["dbeta"][b], ref["dbeta"], ref["ddbeta"], _name(dtype))
            _check(f"bn_bwd dgamma{b} {tag}", got["dgamma"][b], ref["dgamma"][b], ref["ddgamma"][b], _name(dtype))
            _check(f"bn_bwd dz{b} {tag}", got["dz"][b], ref["dz"][b], ref["ddz"][b])
        if two:
            assert torch.equal(got["dbeta"][0], got["dbeta"][1])
        if rpb == 0:                      # without the ReLU mask (the stem's BN is followed by the max-pool's gradient, not by y)
            got = _run_bwd(br, src, None, want_g=False)
            ref = ck.bn_bwd(br, y=None, **src)
            _check(f"bn_bwd dz0 no mask {tag}", got["dz"][0], ref["dz"][0], ref["ddz"][0])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,C", PLANS, ids=PLAN_IDS)
def test_bn_backward_sums_exact(M, C, dtype):
    """integer inputs (clf_kernels_common.bwd_exact_inputs): dbeta and dgamma are exact in f32 in any order, so one dropped or doubled row
    anywhere changes them"""
    e = ck.bwd_exact_inputs(M, C, M + C, DEV)
    gamma = torch.ones(C, device=DEV)
    br = [(e["z"].to(dtype), e["mean"], e["rstd"], gamma), (e["z2"].to(dtype), e["mean2"], e["rstd"], gamma)]
    src, y = dict(dy=e["dy"].to(dtype)), e["y"].to(dtype)
    ref = ck.bn_bwd(br, y=y, **src)
    for nb in (1, 2):
        got = _run_bwd(br[:nb], src, y, want_g=True)
        for b in range(nb):
            assert torch.equal(got["dbeta"][b].double(), ref["dbeta"]), (nb, b)
            assert torch.equal(got["dgamma"][b].double(), ref["dgamma"][b]), (nb, b)
        assert torch.equal(got["g"].double(), ref["g"])
    if M > 8:
        assert bool((ref["dbeta"] != 0).any()) and bool((ref["dgamma"][1] != 0).any())


# ------------------------------------------------------------------------------------------------------------- max-pool
def _same_with_nans(out, ref):
    """bit for bit the reference (rounded once to the result's type: a pure move needs no rounding), NaN at the same positions"""
    o, r = out.double().cpu(), ref.to(out.dtype).double().cpu()
    return torch.equal(torch.isnan(o), torch.isnan(r)) and torch.equal(torch.nan_to_num(o, 123.0), torch.nan_to_num(r, 123.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W,C", ck.POOL_SHAPES)
def test_maxpool_forward_exact_with_nan_and_inf(B, H, W, C, dtype):
    """torch's rule, `val > max or isnan(val)`: a NaN reaches the output of every window that holds it, whatever else the window holds"""
    x = ck.pool_input(B, H, W, C, 1).to(dtype)
    want = ck.maxpool_fwd(x)
    assert bool(torch.isnan(want).any()) and bool((want == -ck.INF).any())
    y = _ops().maxpool3x3s2(x.to(DEV))
    assert _same_with_nans(y, want), f"{int((torch.isnan(y.cpu()) != torch.isnan(want)).sum())} NaN positions differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,H,W,C", ck.POOL_SHAPES)
def test_maxpool_backward_with_nan_and_inf(B, H, W, C, dtype):
    x = ck.pool_input(B, H, W, C, 1).to(dtype)
    dy = torch.randn((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), generator=torch.Generator().manual_seed(2)).to(dtype)
    dx = _ops().maxpool3x3s2_bwd(dy.to(DEV), x.to(DEV)).cpu()
    ref, bound, ref32 = ck.maxpool_bwd(dy, x)
    if dtype == torch.float32:
        assert torch.equal(dx, ref32)
    _check(f"maxpool_bwd {B}x{H}x{W}x{C}", dx, ref, bound)


# ------------------------------------------------------------------------------------------------------------- stride-2 scatter
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_stuff2_add_exact(dtype):
    for B, H, W, C in ((2, 9, 6, 12), (2, 8, 7, 12), (1, 1, 5, 4), (3, 4, 1, 8), (1, 1, 1, 4)):
        dst = _randn((B, H, W, C), H * 10 + W, dtype)
        src = _randn((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), H * 10 + W + 1, dtype)
        want = dst.float().clone()
        want[:, ::2, ::2, :] += src.float()
        got = _ops().stuff2_add(src, dst.clone())
        assert torch.equal(got, want.to(dtype)), (B, H, W, C)


# ------------------------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_bce_bounded(B):
    for zmax in (15.0, 4.0):              # at 15 the bound carries what f32 loses in 1 - sigmoid(z); at 4 it is a few ulp of the loss
        g = torch.Generator(device=DEV).manual_seed(B)
        z = (torch.rand(B, generator=g, device=DEV) * 2 - 1) * zmax
        if B > 2:
            z[0], z[B - 1] = zmax, -zmax
        t = (torch.arange(B, device=DEV) % 2).float()
        loss, dz = _ops().bce_sigmoid(z, t)
        r = ck.bce(z, t)
        _check(f"bce loss B={B} |z|<={zmax:g}", loss[0], r["loss"], r["dloss"])
        _check(f"bce dlogit B={B} |z|<={zmax:g}", dz, r["dlogit"], r["ddlogit"])


def test_bce_saturated_matches_torch_float32():
    """|z| up to 40, where the clamps and f32's 1 - p = 0 are active and float64 is no reference: torch's float32 result, as
    test_clf_train_gpu.py's test, at a B whose stride loop runs three times"""
    z = torch.cat([torch.linspace(-40, 40, 595), torch.tensor([0.0, 17.0, -17.0, 30.0, -30.0])])
    y = (torch.arange(z.numel()) % 2).float()
    assert z.numel() == 600
    zt = z.clone().requires_grad_(True)
    loss = F.binary_cross_entropy(torch.sigmoid(zt), y)
    loss.backward()
    got, dz = _ops().bce_sigmoid(z.to(DEV), y.to(DEV))
    print(f"saturated BCE: loss off by {abs(got.item() - loss.item()):.3e}; dlogit off by {(dz.cpu() - zt.grad).abs().max().item():.3e}")
    assert abs(got.item() - loss.item()) <= 1e-5 * max(1.0, abs(loss.item())), (got.item(), loss.item())
    torch.testing.assert_close(dz.cpu(), zt.grad, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------- im2col
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,C,H,W,KH,KW,stride,pad", [(2, 3, 9, 11, 7, 7, 2, 3), (1, 3, 1, 1, 7, 7, 2, 3), (2, 2, 6, 7, 3, 5, 1, 0),
                                                      (1, 5, 8, 9, 3, 3, 2, 1)])
def test_im2col_exact(B, C, H, W, KH, KW, stride, pad, dtype):
    x = _randn((B, C, H, W), 1)
    K = C * KH * KW
    want = ck.im2col(x, KH, KW, stride, pad)
    for ldk in (K, K + 5):
        cols, Ho, Wo = _ops().im2col_nchw(x, KH, KW, stride, pad, ldk, dtype)
        assert cols.shape == (B * Ho * Wo, ldk) and want.shape == (B * Ho * Wo, K)
        assert torch.equal(cols[:, :K], want.to(dtype))               # a move and one cast
        assert ldk == K or float(cols[:, K:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("Co,K,ldk", [(1, 1, 4), (16, 27, 32), (3, 300, 304), (5, 577, 577)])
def test_bn_fold_bounded(Co, K, ldk, dtype):
    ops = _ops()
    w = _randn((Co, K), 1)
    g, b, m, v = _randn((Co,), 2, shift=0.3), _randn((Co,), 3), _randn((Co,), 4), _randn((Co,), 5).abs() + 0.3
    wf, bf = ops.bn_fold(w, g, b, m, v, 1e-5, ldk, dtype)
    rw, dw, rb, db = ck.bn_fold(w, g, b, m, v, ck.EPS_BN32)
    _check(f"bn_fold weights {Co}x{K}", wf[:, :K], rw, dw)
    _check(f"bn_fold bias {Co}x{K}", bf, rb, db, _name(dtype))
    assert ldk == K or float(wf[:, K:].float().abs().max()) == 0.0
    # the trainer's packing call: unit scale, zero shift -> the weights themselves
    one, zero = torch.ones(Co, device=DEV), torch.zeros(Co, device=DEV)
    wf, bf = ops.bn_fold(w, one, zero, zero, one, 0.0, ldk, dtype)
    assert torch.equal(wf[:, :K], w.to(dtype)) and torch.equal(bf, zero)
    assert ldk == K or float(wf[:, K:].float().abs().max()) == 0.0
