"""unmore_amd.mask_head without a GPU: the parameters' names and shapes, checkpoint loading, the argument checks, and -- in float64
on the host -- the (ky,kx,co) column order and the (2y + ky, 2x + kx) scatter the tail kernels are written against, pinned to torch's
own conv_transpose2d / conv2d through packs' own packers (ops.permute4 replaced by its definition on the host)."""
import pytest
import torch
import torch.nn.functional as F

import mask_head_common as mc

RECIPE_KEYS = {
    **{f"mask_fcn{k}.weight": (256, 256, 3, 3) for k in (1, 2, 3, 4)}, **{f"mask_fcn{k}.bias": (256,) for k in (1, 2, 3, 4)},
    "deconv.weight": (256, 256, 2, 2), "deconv.bias": (256,), "predictor.weight": (1, 256, 1, 1), "predictor.bias": (1,),
}


def _head(*a, **kw):
    from unmore_amd.mask_head import MaskRCNNConvUpsampleHead
    return MaskRCNNConvUpsampleHead(*a, **kw)


def test_state_dict_has_the_reference_names_and_shapes():
    sd = _head().state_dict()
    assert len(sd) == 12 and {k: tuple(v.shape) for k, v in sd.items()} == RECIPE_KEYS
    assert all(v.dtype == torch.float32 for v in sd.values())
    small = _head(64, conv_dims=(128, 64, 192))
    assert {k: tuple(v.shape) for k, v in small.state_dict().items()} == {
        "mask_fcn1.weight": (128, 64, 3, 3), "mask_fcn1.bias": (128,), "mask_fcn2.weight": (64, 128, 3, 3), "mask_fcn2.bias": (64,),
        "deconv.weight": (64, 192, 2, 2), "deconv.bias": (192,), "predictor.weight": (1, 192, 1, 1), "predictor.bias": (1,)}


def test_initialisation_is_the_reference_s():
    torch.manual_seed(5)
    h = _head()
    sd = h.state_dict()
    assert all(float(sd[k].abs().max()) == 0.0 for k in sd if k.endswith(".bias"))
    # c2_msra_fill: kaiming_normal_(fan_out, relu): std = sqrt(2 / (out_channels * kh * kw)); ConvTranspose2d's size(0) is its input count
    for name, fan_out in (("mask_fcn1.weight", 256 * 9), ("mask_fcn4.weight", 256 * 9), ("deconv.weight", 256 * 4)):
        std = float(sd[name].std())
        assert abs(std / (2.0 / fan_out) ** 0.5 - 1) < 0.02, (name, std)
    assert abs(float(sd["predictor.weight"].std()) / 0.001 - 1) < 0.2 and abs(float(sd["predictor.weight"].mean())) < 3e-4


def test_strict_load_of_a_checkpoint_with_and_without_the_prefix():
    src = mc.make_params(256, (256,) * 5, seed=3)
    h = _head()
    assert h.load_state_dict(src, strict=True).missing_keys == []
    assert all(torch.equal(v, src[k]) for k, v in h.state_dict().items())
    prefix = "roi_heads.mask_head."
    ckpt = {prefix + k: v * 2 for k, v in src.items()}
    ckpt["roi_heads.box_head.fc1.weight"] = torch.zeros(3)
    h2 = _head()
    h2.load_state_dict({k[len(prefix):]: v for k, v in ckpt.items() if k.startswith(prefix)}, strict=True)
    assert all(torch.equal(v, src[k] * 2) for k, v in h2.state_dict().items())
    with pytest.raises(RuntimeError):
        _head().load_state_dict({k: v for k, v in src.items() if k != "deconv.bias"}, strict=True)


def _gemm_form(S, C, seed, monkeypatch):
    """(a NCHW, Wd, bd, Wp, bp, D) in float64: D = relu(A . pack_convT(Wd)^T + rep_bias(bd)) with packs' own packers"""
    from unmore_amd import ops, packs
    monkeypatch.setattr(ops, "permute4", mc.permute4_host)
    g = torch.Generator().manual_seed(seed)
    R, ci = 2, 64
    a = torch.randn(R, ci, S, S, generator=g, dtype=torch.float64)
    wd = torch.randn(ci, C, 2, 2, generator=g, dtype=torch.float64) / 8
    bd = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    wp = torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64) / C ** 0.5
    bp = torch.randn(1, generator=g, dtype=torch.float64)
    wt = packs._pack_convT(wd, torch.float64)
    # _rep_bias allocates float32 (the GEMM's bias type); its permute is replayed here into float64 so that the check stays exact
    brep = torch.empty(4 * C, dtype=torch.float64)
    recorded = []
    monkeypatch.setattr(ops, "permute4", lambda *args, **kw: recorded.append(args) or args[1])
    packs._rep_bias(bd, 4)
    monkeypatch.setattr(ops, "permute4", mc.permute4_host)
    (src, _, dims, strides), = recorded
    mc.permute4_host(src, brep, dims, strides)
    assert wt.shape == (4 * C, ci)
    D = F.relu(mc.nhwc(a).reshape(R * S * S, ci) @ wt.t() + brep)
    return a, wd, bd, wp, bp, D


@pytest.mark.parametrize("S,C", [(3, 64), (14, 256)])
def test_tail_logits64_on_the_gemm_form_is_the_layers_composition(S, C, monkeypatch):
    a, wd, bd, wp, bp, D = _gemm_form(S, C, 7, monkeypatch)
    ref = F.conv2d(F.relu(F.conv_transpose2d(a, wd, bd, stride=2)), wp, bp)
    got = mc.tail_logits64(D, wp.reshape(-1), bp, S)
    assert got.shape == ref.shape == (2, 1, 2 * S, 2 * S)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((D == 0).double().mean()) > 0.3 and float((D > 0).double().mean()) > 0.3       # the ReLU mask is about half off
    assert torch.equal(mc.cols_to_map(D, 2, S), F.relu(F.conv_transpose2d(a, wd, bd, stride=2))) or \
        float((mc.cols_to_map(D, 2, S) - F.relu(F.conv_transpose2d(a, wd, bd, stride=2))).abs().max()) < 1e-12
    assert torch.equal(mc.map_to_cols(mc.cols_to_map(D, 2, S), 2, S), D)
    # a wrong tap order or scatter is seen: swap ky and kx
    swapped = D.reshape(-1, 2, 2, C).transpose(1, 2).reshape(D.shape)
    assert float((mc.tail_logits64(swapped, wp.reshape(-1), bp, S) - ref).abs().max()) > 1e-3


@pytest.mark.parametrize("S,C", [(3, 64), (14, 256)])
def test_tail_bwd_is_autograd_s_on_that_composition(S, C, monkeypatch):
    a, wd, bd, wp, bp, D = _gemm_form(S, C, 9, monkeypatch)
    R = 2
    dl = mc.make_dlogits(R, S, 4).double()
    assert float(dl.min()) < 0 < float(dl.max())
    z = F.conv_transpose2d(a, wd, bd, stride=2).requires_grad_(True)            # the deconvolution's pre-activation
    wp_, bp_ = wp.clone().requires_grad_(True), bp.clone().requires_grad_(True)
    F.conv2d(F.relu(z), wp_, bp_).backward(dl)
    G, dwp, dbp = mc.tail_bwd(D, dl, wp.reshape(-1))
    assert G.dtype == D.dtype
    # G forms its product in float32: one float32 rounding of each factor and of the product
    gz = mc.map_to_cols(z.grad, R, S)
    assert float((G - gz).abs().max()) <= 3 * 2.0 ** -24 * float(gz.abs().max())
    assert torch.equal(G == 0, gz == 0) or float(((G == 0) != (gz == 0)).double().mean()) < 1e-6
    assert float((dwp - wp_.grad.reshape(-1)).abs().max()) <= 1e-12 * float(dwp.abs().max())
    assert abs(float(dbp - bp_.grad)) <= 1e-12 * float(dl.abs().sum())
    ab_w, ab_b = mc.tail_bwd_abs(D, dl)
    assert bool((ab_w >= dwp.abs() - 1e-12).all()) and float(ab_b) >= abs(float(dbp))


def test_tail_bwd_rounds_the_float32_product_once():
    g = torch.Generator().manual_seed(1)
    D = torch.randn(2 * 9, 4 * 64, generator=g).relu().bfloat16()
    dl = mc.make_dlogits(2, 3, 2).bfloat16()
    wp = torch.randn(64, generator=g)
    G, _, _ = mc.tail_bwd(D, dl, wp)
    taps = mc._taps(dl, 2, 3).float()
    want = (taps.reshape(18, 4, 1) * wp.reshape(1, 1, 64)).to(torch.bfloat16).reshape(18, 256)
    assert G.dtype == torch.bfloat16 and torch.equal(G[D > 0], want[D > 0]) and bool((G[D <= 0] == 0).all())


@pytest.mark.parametrize("kw", [
    dict(num_classes=2), dict(num_classes=80), dict(conv_norm="GN"), dict(conv_dims=()), dict(conv_dims=(256, 100)),
    dict(conv_dims=(256, 2048)), dict(in_channels=48), dict(in_channels=1088), dict(compute_dtype=torch.float16)])
def test_constructor_argument_errors(kw):
    with pytest.raises(ValueError, match="mask_head"):
        _head(**kw)


def test_layers_argument_errors_come_before_any_launch():
    h = _head(64, conv_dims=(64, 64))
    for bad in (torch.zeros(2, 64, 7), torch.zeros(2, 32, 7, 7), torch.zeros(2, 64, 7, 5), torch.zeros(2, 64, 7, 7, dtype=torch.float16),
                torch.zeros(2, 64, 65, 65), "x"):
        with pytest.raises(ValueError, match="mask_head"):
            h.layers(bad)


def test_cpu_tensors_raise_runtime_error():
    from unmore_amd import mask_head
    h = _head(64, conv_dims=(64, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.layers(torch.zeros(2, 64, 7, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h(torch.zeros(2, 64, 7, 7), [{"pred_boxes": torch.zeros(2, 4)}])
    D, wp, bp = torch.zeros(2 * 9, 256), torch.zeros(64), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mask_head.tail_logits(D, wp, bp, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mask_head.tail_bwd(D, torch.zeros(2, 1, 6, 6), wp, 2, 3)
    for bad in (dict(D=torch.zeros(18, 100)), dict(S=0), dict(S=65), dict(R=3), dict(wp=torch.zeros(32))):
        args = dict(D=D, wp=wp, bp=bp, R=2, S=3)
        args.update(bad)
        with pytest.raises(ValueError, match="mask_head"):
            mask_head.tail_logits(**args)


def test_the_entry_points_are_declared_in_the_header():
    from unmore_amd import _lib as L
    assert {"umr_mask_head_logits", "umr_mask_head_tail_bwd", "umr_mask_head_workspace"} <= set(L.exported_symbols())
    assert L.RESTYPES["umr_mask_head_workspace"] is L._i64 and len(L.ARGTYPES["umr_mask_head_tail_bwd"]) == 14
