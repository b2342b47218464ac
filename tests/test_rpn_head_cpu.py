"""unmore_amd.rpn_head without a GPU: the float64 restatement (tests/rpn_head_common.py) against torch's own conv2d and autograd, the
parameters' names, shapes and initial statistics, checkpoint loading, every argument check, the exported entry points, and -- on the
GPU tests' own shapes -- that each named wrong kernel leaves the bounds those tests assert."""
import pytest
import torch
import torch.nn.functional as F

import rpn_head_common as hc

KEYS = {"conv.weight": (256, 256, 3, 3), "conv.bias": (256,), "objectness_logits.weight": (3, 256, 1, 1), "objectness_logits.bias": (3,),
        "anchor_deltas.weight": (12, 256, 1, 1), "anchor_deltas.bias": (12,)}


def _head(*a, **kw):
    from unmore_amd.rpn_head import StandardRPNHead
    return StandardRPNHead(*a, **kw)


def _rpn(head, nl=2, **kw):
    from unmore_amd import rpn
    from unmore_amd.rpn_head import RPN
    cells = rpn.cell_anchors([[32 * 2 ** k] for k in range(nl)], [0.5, 1.0, 2.0])
    return RPN(head, cells, [4 * 2 ** k for k in range(nl)], **kw)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", hc.TAIL_SHAPES + [(2, 8, 3, ((6, 5), (3, 3)))])
def test_restatement_equals_conv2d_and_autograd_in_float64(shape):
    N, C, A, sizes = shape
    C = min(C, 32)                                                                       # the arithmetic is the same at any width
    sd = {k: v.double().requires_grad_(True) for k, v in hc.make_params(C, A, seed=C + N).items()}
    feats = [f.double().requires_grad_(True) for f in hc.make_features(N, C, sizes, seed=N)]
    dlog, ddel = hc.make_grad_maps(N, A, sizes, seed=7)
    hidden = [F.relu(F.conv2d(x, sd["conv.weight"], sd["conv.bias"], padding=1)) for x in feats]
    logits = [F.conv2d(t, sd["objectness_logits.weight"], sd["objectness_logits.bias"]) for t in hidden]
    deltas = [F.conv2d(t, sd["anchor_deltas.weight"], sd["anchor_deltas.bias"]) for t in hidden]
    torch.autograd.backward(logits + deltas, [g.double() for g in dlog + ddel])
    # forward
    mine = [hc.conv3_relu64(x.detach(), sd["conv.weight"].detach(), sd["conv.bias"].detach()) for x in feats]
    for a, b in zip(mine, hidden):
        assert torch.allclose(a, b.detach(), rtol=1e-12, atol=1e-13)
    T = hc.stack_rows(mine)
    assert torch.equal(torch.cat([t.reshape(-1) for t in hc.unstack_rows(T, N, sizes)]), torch.cat([t.reshape(-1) for t in mine]))
    w = [sd[k].detach() for k in ("objectness_logits.weight", "objectness_logits.bias", "anchor_deltas.weight", "anchor_deltas.bias")]
    lg, dl = hc.predict64(T, N, sizes, *w)
    for a, b in zip(lg + dl, logits + deltas):
        assert a.shape == b.shape and torch.allclose(a, b.detach(), rtol=1e-12, atol=1e-13)
    # backward
    G, dwo, dbo, dwd, dbd = hc.predict_bwd64(T, N, sizes, dlog, ddel, w[0], w[2])
    for got, key in ((dwo, "objectness_logits.weight"), (dbo, "objectness_logits.bias"), (dwd, "anchor_deltas.weight"), (dbd, "anchor_deltas.bias")):
        assert torch.allclose(got.reshape(-1), sd[key].grad.reshape(-1), rtol=1e-11, atol=1e-12), key
    dW, db = torch.zeros_like(sd["conv.weight"]), torch.zeros_like(sd["conv.bias"])
    for x, g in zip(feats, hc.unstack_rows(G, N, sizes)):
        dx, dw_l, db_l = hc.conv3_adjoint64(x.detach(), sd["conv.weight"].detach(), g)
        assert torch.allclose(dx, x.grad, rtol=1e-11, atol=1e-12)
        dW += dw_l
        db += db_l
    assert torch.allclose(dW, sd["conv.weight"].grad, rtol=1e-11, atol=1e-12) and torch.allclose(db, sd["conv.bias"].grad, rtol=1e-11, atol=1e-12)
    # the scales bound the values term by term
    s_lg, s_dl = hc.predict_abs64(T, N, sizes, *w)
    assert all(bool((a.abs() <= s * (1 + 1e-12)).all()) for a, s in zip(lg + dl, s_lg + s_dl))
    scales = hc.predict_bwd_abs64(T, N, sizes, dlog, ddel, w[0], w[2])
    assert all(bool((v.abs() <= s * (1 + 1e-12) + 1e-300).all()) for v, s in zip((G, dwo, dbo, dwd, dbd), scales))


# ---------------------------------------------------------------------------------------------------------------- the bounds can fail
def _outside(err, allow):
    return float((err / allow.clamp_min(1e-300)).max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", hc.TAIL_SHAPES)
@pytest.mark.parametrize("mutant", hc.MUTANTS)
def test_every_named_wrong_kernel_leaves_the_bounds(mutant, shape, dtype):
    """the inputs and allowances of test_rpn_head_gpu's kernel tests, the widest allowance any of them grants (float32 gradients into a
    bfloat16 kernel), and the restatement's mutant in place of the device: the worst error / allowance has to be far above 1"""
    N, C, A, sizes = shape
    M = sum(N * h * w for h, w in sizes)
    T = hc.make_hidden(N, C, sizes, seed=100 + N + C).to(dtype)
    sd = hc.make_params(C, A, seed=C + A)
    w = [sd[k].to(dtype).double() if k.endswith("weight") else sd[k].double()
         for k in ("objectness_logits.weight", "objectness_logits.bias", "anchor_deltas.weight", "anchor_deltas.bias")]
    dlog, ddel = hc.make_grad_maps(N, A, sizes, seed=9)
    rounded = dtype == torch.bfloat16
    ref_out = hc.predict64(T, N, sizes, *w)
    bad_out = hc.predict64(T, N, sizes, *w, mutant=mutant)
    s_out = hc.predict_abs64(T, N, sizes, *w)
    worst_fwd = max(_outside((b - r).abs(), hc.out_allowance(C, s, r, dtype))
                    for r, b, s in zip(ref_out[0] + ref_out[1], bad_out[0] + bad_out[1], s_out[0] + s_out[1]))
    ref = hc.predict_bwd64(T, N, sizes, dlog, ddel, w[0], w[2])
    bad = hc.predict_bwd64(T, N, sizes, dlog, ddel, w[0], w[2], mutant=mutant)
    sc = hc.predict_bwd_abs64(T, N, sizes, dlog, ddel, w[0], w[2])
    worst_bwd = _outside((bad[0] - ref[0]).abs(), hc.g_allowance(A, sc[0], ref[0], dtype, rounded))
    wrong_zero = bool(((T.double() <= 0) & (bad[0] != 0)).any())
    for k in (1, 3):
        worst_bwd = max(worst_bwd, _outside((bad[k] - ref[k]).abs(), hc.w_allowance(M, sc[k], rounded)))
    for k in (2, 4):
        worst_bwd = max(worst_bwd, _outside((bad[k] - ref[k]).abs(), hc.w_allowance(M, sc[k], False)))
    print(f"{mutant} {shape} {dtype}: forward worst err / allowance {worst_fwd:.3g}, backward {worst_bwd:.3g}, G != 0 where T <= 0: {wrong_zero}")
    if (mutant == "level_image_offset" and N == 1) or (mutant == "delta_next_anchor" and A == 1):
        assert worst_fwd == 0 and worst_bwd == 0          # one image / one anchor: the mutant has nothing to confuse; the other shapes see it
        return
    if mutant == "relu_ge":
        assert wrong_zero and worst_fwd == 0              # a backward-only fault, caught by the exact-zero check
    else:
        assert worst_fwd > 10 and worst_bwd > 10


# ---------------------------------------------------------------------------------------------------------------- the module
def test_state_dict_has_detectron2_s_six_names_and_shapes():
    sd = _head().state_dict()
    assert len(sd) == 6 and {k: tuple(v.shape) for k, v in sd.items()} == KEYS and all(v.dtype == torch.float32 for v in sd.values())
    small = _head(64, 2)
    assert {k: tuple(v.shape) for k, v in small.state_dict().items()} == {
        "conv.weight": (64, 64, 3, 3), "conv.bias": (64,), "objectness_logits.weight": (2, 64, 1, 1), "objectness_logits.bias": (2,),
        "anchor_deltas.weight": (8, 64, 1, 1), "anchor_deltas.bias": (8,)}
    assert set(_rpn(_head(64)).state_dict()) == {"rpn_head." + k for k in KEYS}


def test_initialisation_is_normal_001_with_zero_biases():
    torch.manual_seed(5)
    sd = _head().state_dict()
    assert all(float(sd[k].abs().max()) == 0.0 for k in sd if k.endswith(".bias"))
    assert abs(float(sd["conv.weight"].std()) / 0.01 - 1) < 0.02 and abs(float(sd["conv.weight"].mean())) < 1e-4
    for k in ("objectness_logits.weight", "anchor_deltas.weight"):
        assert abs(float(sd[k].std()) / 0.01 - 1) < 0.15 and abs(float(sd[k].mean())) < 2e-3, k


def test_strict_load_of_a_detectron2_checkpoint():
    src = hc.make_params(256, 3, seed=3)
    prefix = "proposal_generator.rpn_head."
    ckpt = {prefix + k: v * 2 for k, v in src.items()}
    ckpt["roi_heads.box_head.fc1.weight"] = torch.zeros(3)
    h = _head()
    res = h.load_state_dict({k[len(prefix):]: v for k, v in ckpt.items() if k.startswith(prefix)}, strict=True)
    assert res.missing_keys == [] and res.unexpected_keys == []
    assert all(torch.equal(v, src[k] * 2) for k, v in h.state_dict().items())
    r = _rpn(_head(256))
    r.load_state_dict({"rpn_head." + k: v for k, v in src.items()}, strict=True)
    assert torch.equal(r.rpn_head.anchor_deltas.bias, src["anchor_deltas.bias"])
    with pytest.raises(RuntimeError):
        _head().load_state_dict({k: v for k, v in src.items() if k != "conv.bias"}, strict=True)


def test_argument_errors_are_value_errors_before_any_launch():
    from unmore_amd import rpn_head
    for kw in (dict(num_anchors=4), dict(num_anchors=0), dict(in_channels=96), dict(in_channels=2048), dict(box_dim=5),
               dict(compute_dtype=torch.float16)):
        with pytest.raises(ValueError, match="rpn_head"):
            _head(**kw)
    h = _head(64)
    x = torch.zeros(2, 64, 4, 4)
    for bad in (x, "p2", [], [x] * 9, [x, torch.zeros(3, 64, 2, 2)], [torch.zeros(2, 32, 4, 4)], [x.double()], [torch.zeros(2, 64, 4)]):
        with pytest.raises(ValueError, match="rpn_head"):
            h(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h([x])
    # the kernel wrappers
    T = torch.zeros(2 * 16, 64)
    sd = hc.make_params(64, 3, seed=1)
    w = [sd[k] for k in ("objectness_logits.weight", "objectness_logits.bias", "anchor_deltas.weight", "anchor_deltas.bias")]
    for args in ((T[:, :32].contiguous(), [(4, 4)], 2, *w), (T, [(4, 5)], 2, *w), (T, [(1, 1)] * 9, 2, *w), (T, [(4, 4)], -1, *w),
                 (T.double(), [(4, 4)], 2, *w), (T, [(4, 4)], 2, w[0], w[1], w[2][:8], w[3]),
                 (T, [(4, 4)], 2, torch.zeros(4, 64), torch.zeros(4), torch.zeros(16, 64), torch.zeros(16))):
        with pytest.raises(ValueError, match="rpn_head"):
            rpn_head.predict(*args)
    dlog, ddel = hc.make_grad_maps(2, 3, [(4, 4)], seed=2)
    for maps in ((dlog, ddel[0]), ([dlog[0][:1]], ddel), (dlog, [ddel[0].double()]), ([dlog[0].bfloat16()], ddel)):
        with pytest.raises(ValueError, match="rpn_head"):
            rpn_head.predict_bwd(T, [(4, 4)], 2, maps[0], maps[1], w[0], w[2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rpn_head.predict(T, [(4, 4)], 2, *w)
    # the proposal generator
    r = _rpn(h).train()
    feats = [torch.zeros(1, 64, 8, 8), torch.zeros(1, 64, 4, 4)]
    gt = [{"gt_boxes": torch.zeros(1, 4)}]
    with pytest.raises(ValueError, match="seed"):
        r([(32, 32)], feats, gt)
    for args in (([(32, 32)], feats, None), ([(32, 32)], feats, [{}]), ([(32, 32)], feats[0], gt), ([(32, 32)], feats[:1], gt)):
        with pytest.raises(ValueError, match="rpn_head"):
            r(*args, seed=1)
    with pytest.raises(ValueError, match="rpn_head"):
        _rpn(_head(64, 2))                                                              # three anchors per cell, a head of two
    with pytest.raises(ValueError):
        _rpn(h, pre_nms_topk=1000)


def test_exported_symbols_and_argument_counts():
    from unmore_amd import _lib as L
    for name, n in (("umr_rpn_head_workspace", 3), ("umr_rpn_head_predict", 13), ("umr_rpn_head_predict_bwd", 18)):
        assert name in L.exported_symbols() and len(L.ARGTYPES[name]) == n, name
    assert L.RESTYPES["umr_rpn_head_workspace"] is L._i64
