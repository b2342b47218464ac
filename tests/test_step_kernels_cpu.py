"""tests/step_kernels_common.py checked without a GPU: (1) every float64 restatement equals something independent of it (F.layer_norm,
F.interpolate, autograd, the oracle's loss); (2) every bound can fail: a reference with a named defect, rounded to the kernel's output
type, exceeds it at the named shape; (3) the inputs of the GPU file's exact tests are exact: evaluated in float32 in another order
they give float64's bits; (4) the launch-plan mirrors give the plans the GPU file's shapes are chosen for."""
import pytest
import torch
import torch.nn.functional as F

import step_kernels_common as sk

EPS32 = float(torch.tensor(1e-6, dtype=torch.float32))


def _randn(shape, seed, dtype=torch.float64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _close(a, b, scale=None):
    """float64 against float64 in another order"""
    s = (b.abs().max() if scale is None else scale) + 1e-300
    return float((a - b).abs().max() / s) <= 1e-12


# ------------------------------------------------------------------------------------------------------------- (1) restatements
@pytest.mark.parametrize("M,D", [(1, 8), (7, 264), (9, 1032), (2, 2048)])
def test_layernorm_restatement_matches_torch(M, D):
    x, g, b, dy, dres = _randn((M, D), 1), _randn((D,), 2), _randn((D,), 3), _randn((M, D), 4), _randn((M, D), 5)
    r = sk.ln_fwd(x, g, b, EPS32)
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.layer_norm(xr, (D,), gr, br, eps=EPS32)
    assert _close(r["y"], y.detach())
    assert _close(r["mean"], x.mean(-1)) and _close(r["rstd"], (x.var(-1, unbiased=False) + EPS32).rsqrt())
    y.backward(dy)
    w = sk.ln_bwd(dy, x, g, r["mean"], r["rstd"])
    assert _close(w["dx"], xr.grad) and _close(w["dgamma"], gr.grad) and _close(w["dbeta"], br.grad)
    prior = (_randn((D,), 6), _randn((D,), 7))
    w2 = sk.ln_bwd(dy, x, g, r["mean"], r["rstd"], dres=dres, prior=prior)
    assert _close(w2["dx"], xr.grad + dres) and _close(w2["dgamma"], gr.grad + prior[0]) and _close(w2["dbeta"], br.grad + prior[1])
    for k in ("dy", "dmean", "drstd"):
        assert bool((r[k] > 0).all()) and bool(torch.isfinite(r[k]).all())
    for k in ("ddx", "ddgamma", "ddbeta"):
        assert bool((w2[k] >= w[k]).all()) and bool((w[k] > 0).all())


RESIZE_SHAPES = [(1, 1, 2, 2), (1, 7, 5, 14), (24, 24, 8, 8), (24, 24, 37, 30), (19, 19, 37, 37), (5, 6, 64, 3), (3, 25, 6, 50),
                 (3, 2, 6, 5), (3, 4, 6, 10), (3, 10, 6, 21), (3, 50, 6, 101), (20, 43, 40, 86), (12, 20, 24, 40), (9, 9, 23, 17),
                 (7, 1, 3, 4), (4, 6, 11, 17)]


@pytest.mark.parametrize("align", [True, False], ids=["align", "half_pixel"])
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", RESIZE_SHAPES)
def test_resize_restatement_matches_interpolate_and_autograd(Hi, Wi, Ho, Wo, align):
    x, dy = _randn((2, Hi, Wi, 3), Hi * 100 + Wi), _randn((2, Ho, Wo, 3), Ho * 100 + Wo)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    yr = F.interpolate(xr, size=(Ho, Wo), mode="bilinear", align_corners=align)
    y, by = sk.resize_fwd(x, Ho, Wo, align)
    assert _close(y, yr.detach().permute(0, 2, 3, 1), x.abs().max())
    yr.backward(dy.permute(0, 3, 1, 2))
    dx, bdx = sk.resize_bwd(dy, Hi, Wi, align)
    assert _close(dx, xr.grad.permute(0, 2, 3, 1), dy.abs().max() * (Ho * Wo) / (Hi * Wi) + 1)
    assert _close(sk.resize_fwd(x, Ho, Wo, align, relu=True)[0], yr.detach().permute(0, 2, 3, 1).clamp_min(0), x.abs().max())
    # weights of an output sum to 1; the bounds are positive wherever a tap value is (a down-scaled input pixel may have none)
    for n_in, n_out in ((Hi, Ho), (Wi, Wo)):
        A, E, cnt = sk.axis_matrices(sk.resize_axis(n_in, n_out, align), n_in)
        assert _close(A.sum(1), torch.ones(n_out, dtype=torch.float64)) and bool((A >= 0).all())
        assert bool((E[A > 0] > 0).all())
    assert bool((by > 0).all()) and bool((bdx[dx != 0] > 0).all())


@pytest.mark.parametrize("act", [sk.ACT_NONE, sk.ACT_TANH, sk.ACT_SINE], ids=["none", "tanh", "sine"])
@pytest.mark.parametrize("Cout", [1, 2])
@pytest.mark.parametrize("relu_mask", [False, True])
def test_head_restatement_matches_autograd(act, Cout, relu_mask):
    B, H, W, K = 2, 5, 3, 12
    h, w, b, dout = _randn((B * H * W, K), 1), _randn((Cout, K), 2), _randn((Cout,), 3), _randn((B, Cout, H, W), 4)
    hr, wr, br = h.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = (hr @ wr.t() + br).reshape(B, H, W, Cout).permute(0, 3, 1, 2)
    o = torch.tanh(z) if act == sk.ACT_TANH else (torch.sin(z) if act == sk.ACT_SINE else z)
    out, bound, zz = sk.head_fwd(h, w, b, B, H, W, act)
    assert _close(out, o.detach()) and _close(zz, z.detach()) and bool((bound > 0).all())
    o.backward(dout)
    saved = out if act == sk.ACT_TANH else zz
    r = sk.head_bwd(h, w, dout, saved, act, relu_mask)
    assert _close(r["dh"], hr.grad * ((h > 0) if relu_mask else 1.0)) and _close(r["dw"], wr.grad) and _close(r["db"], br.grad)


LOSS_SWITCHES = [(c, s, g, b) for c in (True, False) for s in (True, False) for g in (True, False) for b in (True, False)]


def _loss_inputs(B, H, W, seed):
    pc, gc = _randn((B, 2, H, W), seed), _randn((B, 2, H, W), seed + 1)
    ps, gs = torch.tanh(_randn((B, 1, H, W), seed + 2)), torch.tanh(_randn((B, 1, H, W), seed + 3))
    sal = (_randn((B, 1, H, W), seed + 4) > 0).double()
    return pc, ps, gc, gs, sal


@pytest.mark.parametrize("B,H,W", [(3, 11, 13), (2, 1, 9), (2, 9, 1), (1, 2, 2)])
@pytest.mark.parametrize("center_l2,sdf_l2,use_grad,use_bce", [s for s in LOSS_SWITCHES if s[0] == s[1] or s[2]])
def test_loss_restatement_matches_the_oracle(B, H, W, center_l2, sdf_l2, use_grad, use_bce):
    from oracle import objectness_oracle as orc
    pc, ps, gc, gs, sal = _loss_inputs(B, H, W, 7)
    pcr, psr = pc.clone().requires_grad_(True), ps.clone().requires_grad_(True)
    has_grad = use_grad and H > 1 and W > 1              # the oracle's mean over an empty interior is NaN; the kernel's term is 0
    total, terms = orc.loss_terms({"center_fields": pcr, "sdf_maps": psr}, gc, gs, sal, "l2" if center_l2 else "l1",
                                  "l2" if sdf_l2 else "l1", has_grad, use_bce)
    (3.0 * total).backward()
    r = sk.loss(pc, ps, gc, gs, sal, center_l2, sdf_l2, use_grad, use_bce, gscale=3.0)
    want = [total.detach(), terms[0].detach(), terms[1].detach(), terms[2].detach() if has_grad else torch.zeros(()),
            terms[-1].detach() if use_bce else torch.zeros(())]
    assert _close(r["out5"], torch.stack([t.double() for t in want]))
    assert _close(r["dpc"], pcr.grad) and _close(r["dps"], psr.grad)
    assert bool((r["dout5"][:3] > 0).all()) and bool((r["ddpc"] >= 0).all()) and bool((r["ddps"] > 0).all())


# ------------------------------------------------------------------------------------------------------------- (2) the bounds can fail
def _exceeds(mutant, ref, bound):
    return int(((mutant.double() - ref).abs() > bound).sum())


@pytest.mark.parametrize("D", [64, 384])
def test_mutant_variance_over_d_minus_1_shows_on_rstd(D):
    x = _randn((9, D), D).bfloat16()
    g, b = torch.ones(D), torch.zeros(D)
    r, m = sk.ln_fwd(x, g, b, EPS32), sk.ln_fwd(x, g, b, EPS32, var_div=D - 1)
    assert _exceeds(m["rstd"].float(), r["rstd"], r["drstd"]) == 9
    assert _exceeds(r["rstd"].float(), r["rstd"], r["drstd"]) == 0          # the reference itself, rounded to f32, is inside


def test_mutant_last_8_channels_left_out_of_the_mean_shows_on_mean():
    D = 2048
    x = _randn((9, D), 5).bfloat16()
    g, b = torch.ones(D), torch.zeros(D)
    r, m = sk.ln_fwd(x, g, b, EPS32), sk.ln_fwd(x, g, b, EPS32, mean_skip_last=8)
    assert _exceeds(m["mean"].float(), r["mean"], r["dmean"]) >= 1
    assert _exceeds(r["mean"].float(), r["mean"], r["dmean"]) == 0


def test_mutant_eps_1e_5_shows_on_rstd_of_rows_of_spread_1e_2():
    D = 384
    x = (1e-2 * _randn((9, D), 6)).float()
    g, b = torch.ones(D), torch.zeros(D)
    r, m = sk.ln_fwd(x, g, b, EPS32), sk.ln_fwd(x, g, b, float(torch.tensor(1e-5, dtype=torch.float32)))
    assert _exceeds(m["rstd"].float(), r["rstd"], r["drstd"]) == 9


# (Wi, Wo, align): scale exactly 0.4; 0.45 and 0.49 with align_corners; x2 with align_corners on both sides of the <8> / <6> switch
THRESHOLDS = [(2, 5, False), (4, 10, False), (10, 21, True), (50, 101, True), (25, 50, True), (26, 52, True)]


@pytest.mark.parametrize("Wi,Wo,align", THRESHOLDS)
@pytest.mark.parametrize("C", [8, 24])
def test_mutant_dropped_lowest_contributor_shows_on_the_adjoint(Wi, Wo, align, C):
    Hi, Ho = 3, 6
    dy = _randn((1, Ho, Wo, C), Wi).bfloat16()
    ref, b = sk.resize_bwd(dy, Hi, Wi, align)
    mut, _ = sk.resize_bwd(dy, Hi, Wi, align, drop_first=True)
    bound = sk.out_bound(ref, b, torch.bfloat16)
    assert _exceeds(mut.bfloat16(), ref, bound) >= 1
    assert _exceeds(ref.bfloat16(), ref, bound) == 0


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(3, 4, 6, 10), (12, 12, 24, 24)])
def test_mutant_missing_clamp_at_zero_shows_on_the_forward(Hi, Wi, Ho, Wo):
    x = _randn((1, Hi, Wi, 8), 3).bfloat16()
    ref, b = sk.resize_fwd(x, Ho, Wo, False)
    mut, _ = sk.resize_fwd(x, Ho, Wo, False, clamp0=False)
    bound = sk.out_bound(ref, b, torch.bfloat16)
    assert _exceeds(mut.bfloat16(), ref, bound) >= 1 and _exceeds(ref.bfloat16(), ref, bound) == 0


@pytest.mark.parametrize("B,H,W,blocks", [(2, 160, 204, 255), (1, 512, 512, 1024)])
def test_mutant_one_dropped_block_shows_on_every_total(B, H, W, blocks):
    assert sk.loss_plan(B * H * W) == (blocks, 1)
    pc, ps, gc, gs, sal = _loss_inputs(B, H, W, 11)
    r = sk.loss(pc, ps, gc, gs, sal, True, False, True, True)
    m = sk.loss(pc, ps, gc, gs, sal, True, False, True, True, drop_block=blocks // 2)
    over = (m["out5"].float().double() - r["out5"]).abs() > r["dout5"]
    assert bool(over.all()), (m["out5"] - r["out5"], r["dout5"])
    assert _exceeds(r["out5"].float(), r["out5"], r["dout5"] + sk.U32 * r["out5"].abs()) == 0


# ------------------------------------------------------------------------------------------------------------- (3) exact inputs
@pytest.mark.parametrize("M,D", [(905, 64), (12293, 64), (905, 1032), (905, 2048)])
def test_layernorm_exact_inputs_are_exact_in_f32(M, D):
    i = sk.ln_exact_inputs(M, D, 3)
    r = sk.ln_bwd(i["dy"], i["x"], i["gamma"], i["mean"], i["rstd"], dres=i["dres"], prior=i["prior"])
    x, dy, g = i["x"].flip(0), i["dy"].flip(0), i["gamma"]                         # float32 throughout, rows in reverse order
    xh = (x - 2.0) * 0.5
    dgamma = i["prior"][0] + (dy * xh).sum(0)
    dbeta = i["prior"][1] + dy.sum(0)
    assert dgamma.dtype == torch.float32 and torch.equal(dgamma.double(), r["dgamma"]) and torch.equal(dbeta.double(), r["dbeta"])
    if D == 64:
        dg = dy * g
        s1, s2 = dg.flip(1).sum(1, keepdim=True) / D, (dg * xh).flip(1).sum(1, keepdim=True) / D
        dx = 0.5 * (dg - s1 - xh * s2) + i["dres"].flip(0)
        assert torch.equal(dx.flip(0).double(), r["dx"])
        assert float(r["ddx"].max()) > 0          # (the bound is not what the exact tests use; it only has to exist)


@pytest.mark.parametrize("Hi,Wi", [(20, 43), (30, 43)])
def test_resize_exact_inputs_are_exact_in_f32_and_in_bf16(Hi, Wi):
    Ho, Wo = 2 * Hi, 2 * Wi
    x, dy = sk.ints((1, Hi, Wi, 8), 7, 1), sk.ints((1, Ho, Wo, 8), 3, 2)
    y, _ = sk.resize_fwd(x, Ho, Wo, False)
    dx, _ = sk.resize_bwd(dy, Hi, Wi, False)
    Ah, _, _ = sk.axis_matrices(sk.resize_axis(Hi, Ho, False), Hi)
    Aw, _, _ = sk.axis_matrices(sk.resize_axis(Wi, Wo, False), Wi)
    assert set(Ah.unique().tolist()) <= {0.0, 0.25, 0.75, 1.0}
    y32 = torch.einsum("pw,bhwc,oh->bopc", Aw.float(), x, Ah.float())              # x first, then y; float32
    dx32 = torch.einsum("pw,bopc,oh->bhwc", Aw.float(), dy, Ah.float())
    assert y32.dtype == torch.float32 and torch.equal(y32.double(), y) and torch.equal(dx32.double(), dx)
    assert torch.equal(y.bfloat16().double(), y) and torch.equal(dx.bfloat16().double(), dx)
    # F.interpolate in float64, the GPU file's reference for these cases, gives the same bits
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.interpolate(xr, size=(Ho, Wo), mode="bilinear", align_corners=False)
    yr.backward(dy.double().permute(0, 3, 1, 2))
    assert torch.equal(yr.detach().permute(0, 2, 3, 1), y) and torch.equal(xr.grad.permute(0, 2, 3, 1), dx)


@pytest.mark.parametrize("M,K,Cout", [(257 * 257, 8, 2), (524288 + 77, 8, 2), (3 * 37 * 41, 1024, 2)])
def test_head_exact_inputs_are_exact_in_f32(M, K, Cout):
    h, w, b, dout = sk.ints((M, K), 3, 1), sk.ints((Cout, K), 2, 2), sk.ints((Cout,), 2, 3), sk.ints((1, Cout, 1, M), 2, 4)
    r = sk.head_bwd(h, w, dout, None, sk.ACT_NONE, True)
    g = dout[0, :, 0, :].t().contiguous()
    dw32 = g.flip(0).t() @ h.flip(0)
    assert dw32.dtype == torch.float32 and torch.equal(dw32.double(), r["dw"]) and torch.equal(g.flip(0).sum(0).double(), r["db"])
    assert torch.equal(((g @ w) * (h > 0)).double(), r["dh"]) and torch.equal(r["dh"].bfloat16().double(), r["dh"])
    out, _, _ = sk.head_fwd(h, w, b, 1, 1, M, sk.ACT_NONE)
    assert torch.equal((h.flip(1) @ w.flip(1).t() + b).double(), out[0, :, 0, :].t())


@pytest.mark.parametrize("l2", [True, False], ids=["l2", "l1"])
def test_loss_exact_inputs_are_exact_in_f32(l2):
    B, H, W = 2, 512, 512
    pc, ps, gc, gs = sk.loss_exact_inputs(B, H, W, 5)
    r = sk.loss(pc, ps, gc, gs, None, l2, l2, False, False, gscale=4.0)
    dc, ds = (pc - gc).flip(0, 2, 3), (ps - gs).flip(0, 2, 3)
    assert set(dc.unique().tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    t0 = ((dc * dc) if l2 else dc.abs()).sum() * torch.tensor(1.0 / (2 * B * H * W))
    t1 = ((ds * ds) if l2 else ds.abs()).sum() * torch.tensor(1.0 / (B * H * W))
    assert t0.dtype == torch.float32 and float(t0) == float(r["out5"][1]) and float(t1) == float(r["out5"][2])
    assert float(t0 + t1) == float(r["out5"][0])
    assert torch.equal(r["dpc"].float().double(), r["dpc"]) and torch.equal(r["dps"].float().double(), r["dps"])


# ------------------------------------------------------------------------------------------------------------- (4) launch plans
def test_plan_mirrors_give_the_plans_the_gpu_file_names():
    bf, f32 = torch.bfloat16, torch.float32
    assert sk.resize_fwd_plan(32, 40, 86, 512, bf) == dict(kernel="rowstream", run=16, gx=22, gy=96, units=96)
    assert sk.resize_fwd_plan(19, 40, 86, 512, bf)["run"] == 8 and 19 * 5 * 22 == 2090
    assert sk.resize_fwd_plan(2, 24, 24, 16, bf)["run"] == 2 and sk.resize_fwd_plan(2, 24, 24, 16, f32)["kernel"] == "generic2"
    assert sk.resize_fwd_plan(2, 24, 24, 12, bf)["kernel"] == "generic1" and sk.resize_fwd_plan(2, 24, 24, 16, bf, ldx=20)["kernel"] == "generic1"
    p = sk.resize_bwd_plan(63, 30, 43, 60, 86, 512, True, bf)
    assert (p["kernel"], p["run"], p["gx"]) == ("rowstream6", 12, 11)
    assert sk.resize_bwd_plan(63, 30, 43, 60, 86, 512, False, bf)["kernel"] == "rowstream8"
    assert sk.resize_bwd_plan(38, 30, 43, 60, 86, 512, True, bf)["run"] == 6
    want = {(2, 5, False): "rowstream8", (4, 10, False): "rowstream8", (10, 21, True): "rowstream8", (50, 101, True): "rowstream6",
            (25, 50, True): "rowstream8", (26, 52, True): "rowstream6"}
    for (Wi, Wo, align), k in want.items():
        assert sk.resize_bwd_plan(1, 3, Wi, 6, Wo, 8, align, bf)["kernel"] == k, (Wi, Wo, align)
    assert sk.resize_bwd_plan(1, 3, 4, 6, 11, 8, False, bf)["kernel"] == "generic2"          # 4 / 11 < 0.4
    assert sk.resize_bwd_plan(1, 3, 4, 6, 10, 8, False, f32)["kernel"] == "generic2"
    assert sk.ln_bwd_plan(300, 256) == (38, 8) and sk.ln_bwd_plan(16 * 256 + 333, 256) == (493, 9) and sk.ln_bwd_plan(48 * 256 + 5, 256) == (492, 25)
    assert sk.ln_reduce_deep(112) == (0, 7) and sk.ln_reduce_deep(113) == (1, 0) and sk.ln_reduce_deep(114) == (1, 0) and sk.ln_reduce_deep(129) == (1, 1)
    assert sk.head_out_blocks(257 * 257) == (259, 256) and sk.head_out_blocks(524288 + 77) == (2041, 257)
    assert sk.head_fwd_grid(65536)[1] == 1 and sk.head_fwd_grid(257 * 257)[1] == 2
    assert sk.loss_plan(429) == (2, 1) and sk.loss_plan(262144) == (1024, 1) and sk.loss_plan(2 ** 19) == (1024, 2)
    assert sk.adam_grid(1000) == (4, 1) and sk.adam_grid(16384 * 256 + 13) == (16384, 2)
