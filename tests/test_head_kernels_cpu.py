"""The float64 restatement the GPU tests of the collapsed head compare against (tests/linear_head_common.py), checked here against
something independent of it: float64 conv2d and autograd.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import linear_head_common as lh

C = 256
SHAPES = [(2, 3, 67), (2, 7, 5)]      # two of the ragged shapes of tests/test_head_kernels_gpu.py


def _case(B, H, W, integer, seed):
    g = torch.Generator().manual_seed(seed)
    if integer:
        r = lambda shape, m: torch.randint(-m, m + 1, shape, generator=g).double()
        return r((B, H, W, C), 3), r((9, C), 2), r((10,), 2), r((B, 1, H, W), 2)
    r = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64)
    return r(B, H, W, C), r(9, C) / 16, r(10), r(B, 1, H, W)


def _conv(x, kw, tb, act):
    """the head as PyTorch states it: one 3x3 cross-correlation 256 -> 1 with zero padding; tap t's bias counts where the tap is inside"""
    B, H, W, _ = x.shape
    K = kw.view(3, 3, C).permute(2, 0, 1)[None].contiguous()                        # [1, C, 3, 3]: K[0, c, ky, kx] = kw[ky*3 + kx][c]
    border = F.conv2d(torch.ones(1, 1, H, W, dtype=torch.float64), tb[:9].view(1, 1, 3, 3), padding=1)
    return lh.act_apply(F.conv2d(x.permute(0, 3, 1, 2), K, padding=1) + border + tb[9], act)


@pytest.mark.parametrize("act", [lh.ACT_NONE, lh.ACT_TANH, lh.ACT_SINE], ids=["none", "tanh", "sine"])
@pytest.mark.parametrize("integer", [True, False], ids=["int", "randn"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_restatement_matches_conv2d_and_autograd(B, H, W, integer, act):
    x, kw, tb, dout = _case(B, H, W, integer, seed=H * 1000 + W)
    xr, kwr, tbr = x.clone().requires_grad_(True), kw.clone().requires_grad_(True), tb.clone().requires_grad_(True)
    y = _conv(xr, kwr, tbr, act)
    out, S, n = lh.fwd(x, kw, tb, act)
    tol = 1e-13 * S                                 # float64 in another order; integers: exact
    assert out.shape == (B, 1, H, W)
    assert bool(((out - y.detach()).abs() <= tol).all())
    if integer and act == lh.ACT_NONE:
        assert torch.equal(out, y.detach())
    # the term counts: (C + 1) per tap inside, plus the constant
    inside = F.conv2d(torch.ones(1, 1, H, W, dtype=torch.float64), torch.ones(1, 1, 3, 3, dtype=torch.float64), padding=1)
    assert torch.equal(n, (inside * (C + 1) + 1).expand(B, 1, H, W))
    if act == lh.ACT_NONE:
        assert bool((S >= out.abs() * (1 - 1e-12)).all())
    if act == lh.ACT_SINE:
        return                                      # no backward for sine
    (y * dout).sum().backward()
    yout = y.detach() if act == lh.ACT_TANH else None
    dx, Sd, nd = lh.bwd_data(dout, yout, kw, act)
    assert nd == (18 if act == lh.ACT_TANH else 9)
    assert bool(((dx - xr.grad).abs() <= 1e-13 * Sd).all())
    R, Sw, nw = lh.bwd_weight(x, dout, yout, act)
    want = torch.cat([kwr.grad.reshape(-1), tbr.grad])          # [G | n | D] = gradients of kw, tb[:9], tb[9]
    assert R.shape == want.shape == (9 * C + 10,)
    assert bool(((R - want).abs() <= 1e-13 * Sw).all())
    assert bool((Sw >= R.abs() * (1 - 1e-12)).all())
    if integer and act == lh.ACT_NONE:
        assert torch.equal(dx, xr.grad) and torch.equal(R, want)
    mono = 2 if act == lh.ACT_TANH else 1
    cnt = torch.tensor([B * (H - abs(t // 3 - 1)) * (W - abs(t % 3 - 1)) for t in range(9)], dtype=torch.float64) * mono
    assert torch.equal(nw[:9 * C].view(9, C), cnt[:, None].expand(9, C)) and torch.equal(nw[9 * C:9 * C + 9], cnt)
    assert nw[-1].item() == B * H * W * mono
    # accumulate: the prior contents are one more term
    prior = torch.randint(-8, 9, dx.shape, generator=torch.Generator().manual_seed(5)).double()
    dx2, Sd2, nd2 = lh.bwd_data(dout, yout, kw, act, prior=prior)
    assert nd2 == nd + 1 and bool(((dx2 - (xr.grad + prior)).abs() <= 1e-13 * Sd2).all())
    assert torch.allclose(Sd2, Sd + prior.abs(), rtol=1e-14, atol=0)


def test_neighbouring_images_do_not_leak():
    """row -1 of image 1 is not row H-1 of image 0: changing one image changes only its own outputs"""
    x, kw, tb, dout = _case(2, 3, 5, True, seed=1)
    out0, _, _ = lh.fwd(x, kw, tb, lh.ACT_NONE)
    x2 = x.clone()
    x2[1] += 1
    out1, _, _ = lh.fwd(x2, kw, tb, lh.ACT_NONE)
    assert torch.equal(out0[0], out1[0]) and not torch.equal(out0[1], out1[1])


@pytest.mark.parametrize("accumulate", [False, True])
def test_small_gemm_restatement_matches_as_strided_matmul(accumulate):
    g = torch.Generator().manual_seed(3)
    M, N, K = 5, 7, 11
    for sa, sb, sc in [((K, 1), (N, 1), (N, 1)), ((1, M), (1, K), (1, M)), ((0, 1), (N, 1), (N, 1)), ((K + 2, 1), (N + 3, 1), (N + 1, 1))]:
        ext = lambda d0, d1, s: 1 + (d0 - 1) * s[0] + (d1 - 1) * s[1]
        A = torch.randn(ext(M, K, sa), generator=g, dtype=torch.float64)
        B = torch.randn(ext(K, N, sb), generator=g, dtype=torch.float64)
        C0 = torch.randn(ext(M, N, sc), generator=g, dtype=torch.float64)
        out, ic, S, n = lh.small_gemm(A, B, C0, M, N, K, sa, sb, sc, accumulate)
        want = C0.clone()
        prod = torch.as_strided(A, (M, K), sa) @ torch.as_strided(B, (K, N), sb)
        view = torch.as_strided(want, (M, N), sc)
        view.copy_(view + prod if accumulate else prod)
        assert torch.allclose(out, want, rtol=1e-13, atol=1e-13) and n == K + int(accumulate)
        assert bool((S >= out[ic].abs() - 1e-12).all())


def test_segsum_restatement_matches_as_strided_sum():
    g = torch.Generator().manual_seed(4)
    B, Nt, D = 3, 4, 5
    x = torch.randn(B * Nt * D, generator=g, dtype=torch.float64)
    out, S, n = lh.segsum(x, B, Nt, D, Nt * D, D)                     # sum over the rows of [B, Nt, D]
    assert torch.allclose(out, x.view(B, Nt, D).sum(1), rtol=1e-14, atol=1e-14) and n == Nt
    prior = torch.randn(Nt, D, generator=g, dtype=torch.float64)
    out, S, n = lh.segsum(x, Nt, B, Nt * D, D, D, prior=prior)        # sum over images
    assert torch.allclose(out, x.view(B, Nt, D).sum(0) + prior, rtol=1e-14, atol=1e-14) and n == B + 1
    assert torch.allclose(S, x.view(B, Nt, D).abs().sum(0) + prior.abs(), rtol=1e-14, atol=1e-14)


def test_half_ulp_bf16():
    v = torch.tensor([0.0, 1.0, 1.5, 2.0, -3.0, 255.0, 0.75], dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.5, 2.0 ** -9], dtype=torch.float64)
    assert torch.equal(lh.half_ulp_bf16(v), want)
    # a value half way between two bf16 numbers is half an ulp from both
    x = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)
    assert abs(x.float().to(torch.bfloat16).double() - x).item() == lh.half_ulp_bf16(x).item()
