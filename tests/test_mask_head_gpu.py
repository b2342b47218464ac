"""unmore_amd.mask_head on the device against the float64 restatement (tests/mask_head_common.py).

Bounds.  The tail kernels sum in float32: a logit is a sum of C + 1 terms, so |logit - ref64| <= 2 * (C + 1) * 2^-24 * (|bp| + sum |D * wp|)
(the n * u bound, doubled), plus one rounding of a bfloat16 output, 2^-8 * |ref64|; dwp and dbp are sums of n = 4 * R * S * S terms,
bound 2 * n * 2^-24 * sum |terms|; G is one float32 product rounded once and must equal the restatement bit for bit.  The GEMM layers
are held to the project's GEMM tolerance (gemm_forms_common.tol) against the float64 layer applied to the device's OWN stored input
(and, backward, its own incoming gradient and masks), with the weights as the device reads them: rounded to the compute type.  End to
end, the device's gradient error against float64 autograd (e_dev) is held against the error of the same chain in torch on the CPU in
the compute type (e_ref): e_dev <= 2 * e_ref + tol.atol * max|ref|; the 2 allows for another summation order inside the GEMMs."""
import types

import numpy as np
import pytest
import torch

import mask_head_common as mc
from gemm_forms_common import tol
from mask_loss_common import blob_masks, jittered_proposals, tight_boxes

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def _dev():
    return torch.device("cuda", 0)


def _out_round(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 0.0


def _close(x, ref, dtype, what):
    """x within tol(dtype) of ref everywhere; prints the largest error against its allowance"""
    t = tol(dtype)
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    assert x.shape == ref.shape, (what, x.shape, ref.shape)
    err, allow = (x - ref).abs(), t["atol"] + t["rtol"] * ref.abs()
    worst = float((err / allow).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, max |ref| {float(ref.abs().max()) if ref.numel() else 0.0:.3e}, "
          f"worst err / allowance {worst:.3f}")
    assert bool(torch.isfinite(x).all()) and worst <= 1.0, what


def _head(cin, dims, dtype, sd=None, **kw):
    from unmore_amd.mask_head import MaskRCNNConvUpsampleHead
    h = MaskRCNNConvUpsampleHead(cin, conv_dims=dims, compute_dtype=dtype, **kw)
    if sd is not None:
        h.load_state_dict(sd, strict=True)
    return h.to(_dev())


# ---------------------------------------------------------------------------------------------------------------- 1. the tail kernels
# (R, S, C); the last: M = 4116 rows, 17 workgroups of the backward, so the finishing sum's wave 0 adds two partial records
TAIL_SHAPES = [(3, 3, 64), (5, 14, 256), (1, 1, 1024), (21, 14, 64)]


class Tail:
    """one shape and type: the inputs, the float64 reference, and every output of both kernels (twice), on the host"""

    def __init__(self, R, S, C, dtype):
        from unmore_amd import mask_head
        g = torch.Generator().manual_seed(100 + R + S + C)
        M = R * S * S
        self.R, self.S, self.C, self.dtype, self.M = R, S, C, dtype, M
        self.D = torch.randn(M, 4 * C, generator=g).relu().to(dtype)                   # about half of the mask off
        self.wp = torch.randn(C, generator=g) / C ** 0.5
        self.bp = torch.randn(1, generator=g)
        self.dl = mc.make_dlogits(R, S, 7).to(dtype)
        dev = _dev()
        d, wp, bp = self.D.to(dev), self.wp.to(dev), self.bp.to(dev)
        self.out = {}
        for rep in (0, 1):
            for out_f32 in (False, True):
                for sig in (False, True):
                    self.out[("logits", out_f32, sig, rep)] = mask_head.tail_logits(d, wp, bp, R, S, out_f32=out_f32, sigmoid=sig).cpu()
            for dl_f32 in (False, True):
                dd = d.clone()
                dlv = self.dl.float() if dl_f32 else self.dl
                G, dwp, dbp = mask_head.tail_bwd(dd, dlv.to(dev), wp, R, S)
                assert G.data_ptr() == dd.data_ptr()
                self.out[("bwd", dl_f32, rep)] = (G.cpu(), dwp.cpu(), dbp.cpu())
        assert torch.equal(d.cpu(), self.D)                                             # tail_logits only reads D


@pytest.fixture(scope="module")
def tails():
    cache = {}

    def get(shape, name):
        if (shape, name) not in cache:
            cache[(shape, name)] = Tail(*shape, DTYPES[name])
        return cache[(shape, name)]
    return get


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_logits_within_the_float32_sum_bound(tails, shape, name):
    t = tails(shape, name)
    ref = mc.tail_logits64(t.D, t.wp, t.bp, t.S)
    scale = mc.tail_abs64(t.D, t.wp, t.bp, t.S)
    for out_f32 in (False, True):
        got = t.out[("logits", out_f32, False, 0)]
        assert got.dtype == (torch.float32 if out_f32 else t.dtype) and tuple(got.shape) == (t.R, 1, 2 * t.S, 2 * t.S)
        allow = 2 * (t.C + 1) * U32 * scale + (0.0 if out_f32 else _out_round(t.dtype)) * ref.abs()
        err = (got.double() - ref).abs()
        print(f"{shape} {name} out_f32={out_f32}: max |err| {float(err.max()):.3e}, worst err / allowance {float((err / allow).max()):.3f}")
        assert bool((err <= allow).all())
    assert float(ref.min()) < 0 < float(ref.max())


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_sigmoid_is_one_rounding_from_the_float32_logit(tails, shape, name):
    t = tails(shape, name)
    ref = torch.sigmoid(t.out[("logits", True, False, 0)].double())
    for out_f32 in (False, True):
        got = t.out[("logits", out_f32, True, 0)]
        u = U32 if out_f32 or t.dtype == torch.float32 else 2.0 ** -8
        err = (got.double() - ref).abs()
        print(f"{shape} {name} out_f32={out_f32}: worst err / (u * p) {float((err / (u * ref)).max()):.3f}")
        assert got.dtype == (torch.float32 if out_f32 else t.dtype) and bool((err <= u * ref).all())


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_bwd_g_is_bit_equal_and_the_sums_are_within_their_bounds(tails, shape, name):
    t = tails(shape, name)
    n = 4 * t.M
    for dl_f32 in (False, True):
        dl = t.dl.float() if dl_f32 else t.dl
        G, dwp, dbp = t.out[("bwd", dl_f32, 0)]
        G_ref, dwp_ref, dbp_ref = mc.tail_bwd(t.D, dl, t.wp)
        assert G.dtype == t.dtype and torch.equal(G.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32),
                                                 G_ref.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32))
        assert 0.3 < float((G == 0).double().mean()) < 0.7
        sw, sb = mc.tail_bwd_abs(t.D, dl)
        ew, eb = (dwp.double() - dwp_ref).abs(), abs(float(dbp.double() - dbp_ref))
        print(f"{shape} {name} dl_f32={dl_f32}: dwp worst err / allowance {float((ew / (2 * n * U32 * sw).clamp_min(1e-300)).max()):.4f}, "
              f"dbp {eb / (2 * n * U32 * float(sb)):.4f}")
        assert dwp.dtype == dbp.dtype == torch.float32 and tuple(dwp.shape) == (t.C,) and tuple(dbp.shape) == (1,)
        assert bool((ew <= 2 * n * U32 * sw).all()) and eb <= 2 * n * U32 * float(sb)


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_kernels_give_the_same_bytes_twice(tails, shape, name):
    t = tails(shape, name)
    for key, v in t.out.items():
        if key[-1] != 0:
            continue
        again = t.out[key[:-1] + (1,)]
        for a, b in zip(v if isinstance(v, tuple) else (v,), again if isinstance(again, tuple) else (again,)):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), key


def test_tail_entry_points_refuse_bad_arguments_without_a_launch():
    import ctypes
    from unmore_amd import _lib as L
    lib = L.lib()
    dev = _dev()
    D = torch.zeros(18, 256, dtype=torch.bfloat16, device=dev)
    wp, bp, out = torch.zeros(64, device=dev), torch.zeros(1, device=dev), torch.zeros(2, 1, 6, 6, dtype=torch.bfloat16, device=dev)
    dwp, ws = torch.zeros(65, device=dev), torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    INVALID, UNSUPPORTED = -1, -2

    def logits(D_=p(D), wp_=p(wp), bp_=p(bp), out_=p(out), R=2, S=3, C=64, dtype=L.BF16):
        return lib.umr_mask_head_logits(D_, wp_, bp_, out_, R, S, C, dtype, 0, 0, None)

    def bwd(D_=p(D), dl_=p(out), wp_=p(wp), dwp_=p(dwp), R=2, S=3, C=64, dtype=L.BF16, ws_=p(ws), nbytes=1 << 16, phases=3):
        return lib.umr_mask_head_tail_bwd(D_, dl_, 0, wp_, dwp_, p(bp), ws_, nbytes, R, S, C, dtype, phases, None)

    assert logits() == 0 and bwd() == 0
    for call in (logits, bwd):
        assert call(C=96) == UNSUPPORTED and call(C=2048) == UNSUPPORTED and call(C=0) == UNSUPPORTED
        assert call(S=0) == UNSUPPORTED and call(S=65) == UNSUPPORTED
        assert call(D_=None) == INVALID and call(wp_=None) == INVALID and call(dtype=7) == INVALID and call(R=-1) == INVALID
        assert b"mask_head" in lib.umr_last_error_string()
    assert logits(out_=None) == INVALID and logits(bp_=None) == INVALID
    assert bwd(dl_=None) == INVALID and bwd(dwp_=None) == INVALID and bwd(ws_=None) == INVALID and bwd(nbytes=16) == INVALID
    assert bwd(phases=0) == INVALID and bwd(phases=4) == INVALID
    assert logits(D_=None, R=0) == 0 and bwd(D_=None, dl_=None, R=0) == 0                  # R == 0: a successful no-op
    assert lib.umr_mask_head_workspace(980, 256) == 4 * 257 * 4 and lib.umr_mask_head_workspace(0, 64) == 65 * 4
    assert lib.umr_mask_head_workspace(10, 96) == -1 and lib.umr_mask_head_workspace(-1, 64) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2, 3. layer by layer
LAYER_CASES = {"3x14x64-bf16": (3, 14, 64, "bf16"), "3x14x64-f32": (3, 14, 64, "f32"), "37x14x256-bf16": (37, 14, 256, "bf16")}


class Run:
    """one forward and backward of the module with its stored activations and gradients, on the host"""

    def __init__(self, R, S, C, name):
        dtype = DTYPES[name]
        self.R, self.S, self.C, self.dtype, self.nconv = R, S, C, dtype, 4
        self.sd = mc.make_params(C, (C,) * 5, seed=C + R)
        head = _head(C, (C,) * 5, dtype, self.sd)
        self.x = mc.make_features(R, C, S, seed=R)
        x = self.x.to(_dev()).requires_grad_(True)
        keep = {}
        logits = head.layers(x, _keep=keep)
        self.dl = mc.make_dlogits(R, S, 11).to(dtype)
        logits.backward(self.dl.to(_dev()))
        self.logits = logits.detach().cpu()
        self.acts = [a.cpu() for a in keep["acts"]]                    # NHWC: the input in the compute type, then the four conv outputs
        self.D = keep["D"].cpu()
        self.kept = {k: (None if v is None else v.cpu()) for k, v in keep["grads"].items()}
        self.gx = x.grad.cpu()
        self.grads = {k: p.grad.cpu() for k, p in head.named_parameters()}
        self.w = {k: v.to(dtype).double() if k.endswith("weight") and not k.startswith("predictor") else v.double() for k, v in self.sd.items()}


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Run(*LAYER_CASES[case])
        return cache[case]
    return get


@pytest.mark.parametrize("case", sorted(LAYER_CASES))
def test_forward_layer_by_layer(runs, case):
    r = runs(case)
    R, S, C = r.R, r.S, r.C
    assert tuple(r.acts[0].shape) == (R, S, S, C) and r.acts[0].dtype == r.dtype
    assert torch.equal(r.acts[0], mc.nhwc(r.x).to(r.dtype))                             # NCHW -> NHWC and the cast, exactly
    for k in range(4):
        ref = mc.nhwc(mc.conv_relu(mc.nchw(r.acts[k].double()), r.w[f"mask_fcn{k + 1}.weight"], r.w[f"mask_fcn{k + 1}.bias"]))
        _close(r.acts[k + 1], ref, r.dtype, f"{case} mask_fcn{k + 1}")
        assert 0.2 < float((r.acts[k + 1] == 0).double().mean()) < 0.8
    ref = mc.map_to_cols(mc.deconv_relu(mc.nchw(r.acts[4].double()), r.w["deconv.weight"], r.w["deconv.bias"]), R, S)
    _close(r.D, ref, r.dtype, f"{case} deconv")
    assert 0.2 < float((r.D == 0).double().mean()) < 0.8
    wp, bp = r.sd["predictor.weight"].reshape(-1), r.sd["predictor.bias"]
    ref = mc.tail_logits64(r.D, wp, bp, S)
    allow = 2 * (C + 1) * U32 * mc.tail_abs64(r.D, wp, bp, S) + _out_round(r.dtype) * ref.abs()
    assert r.logits.dtype == r.dtype and bool(((r.logits.double() - ref).abs() <= allow).all())


@pytest.mark.parametrize("case", sorted(LAYER_CASES))
def test_backward_layer_by_layer(runs, case):
    r = runs(case)
    R, S, C, n = r.R, r.S, r.C, 4 * r.R * r.S * r.S
    wp = r.sd["predictor.weight"].reshape(-1)
    G_ref, dwp_ref, dbp_ref = mc.tail_bwd(r.D, r.dl, wp)
    G = r.kept["G"]
    assert torch.equal(G.view(torch.int16 if r.dtype == torch.bfloat16 else torch.int32),
                       G_ref.view(torch.int16 if r.dtype == torch.bfloat16 else torch.int32))
    sw, sb = mc.tail_bwd_abs(r.D, r.dl)
    assert bool(((r.grads["predictor.weight"].reshape(-1).double() - dwp_ref).abs() <= 2 * n * U32 * sw).all())
    assert abs(float(r.grads["predictor.bias"].double() - dbp_ref)) <= 2 * n * U32 * float(sb)
    da, dw, db = mc.deconv_adjoint64(r.acts[4], r.w["deconv.weight"], r.w["deconv.bias"], G, mask_of=r.acts[4])
    _close(r.kept["da4"].reshape(R, S, S, C), da, r.dtype, f"{case} deconv data gradient")
    _close(r.grads["deconv.weight"], dw, r.dtype, f"{case} deconv.weight")
    _close(r.grads["deconv.bias"], db, r.dtype, f"{case} deconv.bias")
    for k in range(4, 0, -1):
        dz = r.kept[f"da{k}"].reshape(R, S, S, C)
        da, dw, db = mc.conv_adjoint64(r.acts[k - 1], r.w[f"mask_fcn{k}.weight"], r.w[f"mask_fcn{k}.bias"], dz,
                                       mask_of=(r.acts[k - 1] if k > 1 else None))
        _close(r.kept[f"da{k - 1}"].reshape(R, S, S, C), da, r.dtype, f"{case} mask_fcn{k} data gradient")
        _close(r.grads[f"mask_fcn{k}.weight"], dw, r.dtype, f"{case} mask_fcn{k}.weight")
        _close(r.grads[f"mask_fcn{k}.bias"], db, r.dtype, f"{case} mask_fcn{k}.bias")
    assert r.gx.dtype == torch.float32 and torch.equal(r.gx, mc.nchw(r.kept["da0"].reshape(R, S, S, C)).float())   # NHWC -> NCHW, exactly
    assert all(g.dtype == torch.float32 and g.shape == r.sd[k].shape for k, g in r.grads.items())


# ---------------------------------------------------------------------------------------------------------------- 4. with the loss
def _instances(seed=3, objects=False):
    """2 images of 64 x 96 with 3 and 2 blob masks, proposals jittered from the masks' boxes, scores in (0, 1)"""
    rng = np.random.RandomState(seed)
    items = []
    for G in (3, 2):
        masks = blob_masks(rng, 64, 96, G)
        boxes = tight_boxes(masks)
        jit = (rng.uniform(-0.1, 0.1, boxes.shape) * np.stack([boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]] * 2, axis=1)).astype(np.float32)
        item = {"gt_masks": torch.from_numpy(masks).cuda(), "proposal_boxes": torch.from_numpy(boxes + jit).cuda(),
                "gt_scores": torch.from_numpy(rng.uniform(0.05, 0.95, G).astype(np.float32)).cuda()}
        if objects:
            item = types.SimpleNamespace(gt_masks=types.SimpleNamespace(tensor=item["gt_masks"]),
                                         proposal_boxes=types.SimpleNamespace(tensor=item["proposal_boxes"]), gt_scores=item["gt_scores"])
        items.append(item)
    return items


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_end_to_end_with_the_loss(name):
    from unmore_amd import mask_loss
    dtype, C, S, R = DTYPES[name], 64, 14, 5
    sd = mc.make_params(C, (C,) * 5, seed=21)
    head = _head(C, (C,) * 5, dtype, sd, loss_weight=2.0).train()
    inst = _instances()
    x0 = mc.make_features(R, C, S, seed=8)
    x = x0.cuda().requires_grad_(True)
    loss = head(x, inst)["loss_mask"]
    loss.backward()
    stats = {}
    weights = torch.cat([i["gt_scores"] for i in inst])
    mask_loss.mask_rcnn_loss_weighted(torch.zeros(R, 1, 2 * S, 2 * S, device=_dev()), inst, weights, stats=stats)
    targets, w = stats["targets"].cpu(), weights.cpu()
    assert 0.1 < float(targets.double().mean()) < 0.9

    def chain(to, post):
        leaves = {k: v.clone().to(to).requires_grad_(True) for k, v in sd.items()}
        xl = x0.clone().to(to).requires_grad_(True)
        logits = mc.head_logits(post(xl), {k: (post(v) if k.endswith("weight") and not k.startswith("predictor") else v)
                                           for k, v in leaves.items()}, 4, post)
        val = mc.weighted_bce(logits, targets, w) * 2.0
        val.backward()
        return val.detach(), {**{k: v.grad for k, v in leaves.items()}, "x": xl.grad}

    loss64, g64 = chain(torch.float64, lambda t: t)
    _, gref = chain(torch.float32, lambda t: mc.round_to(t, dtype))
    t = tol(dtype)
    print(f"{name}: loss {float(loss.detach()):.8f}, float64 {float(loss64):.8f}")
    assert loss.dtype == torch.float32 and abs(float(loss.detach()) - float(loss64)) <= t["atol"] + t["rtol"] * abs(float(loss64))
    gdev = {**{k: p.grad.cpu() for k, p in head.named_parameters()}, "x": x.grad.cpu()}
    worst = 0.0
    for k in sorted(g64):
        ref = g64[k]
        e_dev, e_ref = float((gdev[k].double() - ref).abs().max()), float((gref[k].double() - ref).abs().max())
        allow = 2 * e_ref + t["atol"] * float(ref.abs().max())
        worst = max(worst, e_dev / allow)
        print(f"{name} {k}: e_dev {e_dev:.3e}, e_ref {e_ref:.3e}, max |ref| {float(ref.abs().max()):.3e}, e_dev / allowance {e_dev / allow:.3f}")
    for k in sorted(g64):
        ref = g64[k]
        e_dev, e_ref = float((gdev[k].double() - ref).abs().max()), float((gref[k].double() - ref).abs().max())
        assert gdev[k].dtype == torch.float32 and e_dev <= 2 * e_ref + t["atol"] * float(ref.abs().max()), k
    # the unweighted loss of the other switch
    head2 = _head(C, (C,) * 5, dtype, sd, use_soft_targets=False).train()
    plain = head2(x0.cuda(), inst)["loss_mask"]
    ref = mc.weighted_bce(mc.head_logits(x0.double(), {k: v.double() for k, v in sd.items()}, 4), targets, torch.ones(R))
    assert abs(float(plain.detach()) - float(ref)) <= t["atol"] + t["rtol"] * abs(float(ref))


# ---------------------------------------------------------------------------------------------------------------- 5. eval mode
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_eval_mode_attaches_the_probabilities_per_image(name):
    dtype, C, S = DTYPES[name], 64, 14
    head = _head(C, (C, C, C), dtype, mc.make_params(C, (C, C, C), seed=4)).eval()
    x = mc.make_features(5, C, S, seed=9).cuda().requires_grad_(True)
    logits = head.layers(x).detach()
    ref = torch.sigmoid(logits.double())
    # float32: the same float32 logit, one rounding of the probability.  bfloat16: the probability is formed from the float32 logit,
    # `logits` is that logit rounded (bfloat16 keeps 8 significant bits: 2^-8 relative; sigmoid' <= 1/4), and the probability is rounded
    # once to bfloat16
    allow = U32 * ref if dtype == torch.float32 else 2.0 ** -8 * ref + 1.01 * 2.0 ** -8 * logits.double().abs() / 4
    boxes = [torch.zeros(3, 4, device=_dev()), torch.zeros(2, 4, device=_dev())]
    as_dicts = [{"pred_boxes": b} for b in boxes]
    as_objects = [types.SimpleNamespace(pred_boxes=types.SimpleNamespace(tensor=b)) for b in boxes]
    out_d, out_o = head(x, as_dicts), head(x, as_objects)
    assert out_d is as_dicts and out_o is as_objects
    got_d, got_o = [i["pred_masks"] for i in out_d], [i.pred_masks for i in out_o]
    assert [tuple(g.shape) for g in got_d] == [(3, 1, 2 * S, 2 * S), (2, 1, 2 * S, 2 * S)]
    for got in (got_d, got_o):
        cat = torch.cat(got)
        assert cat.dtype == dtype and not cat.requires_grad and bool(((cat.double() - ref).abs() <= allow).all())
        assert float(cat.min()) > 0 and float(cat.max()) < 1
    assert torch.equal(torch.cat(got_d), torch.cat(got_o))
    assert x.grad is None and all(p.grad is None for p in head.parameters())
    with pytest.raises(ValueError, match="mask_head"):
        head(x, [{"pred_boxes": boxes[0]}])


# ---------------------------------------------------------------------------------------------------------------- 6. R == 0
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_no_proposals_give_a_zero_loss_and_zero_gradients(name):
    dtype, C = DTYPES[name], 64
    head = _head(C, (C, C), dtype).train()
    x = torch.zeros(0, C, 14, 14, device=_dev(), requires_grad=True)
    inst = [{"gt_masks": torch.zeros(1, 64, 96, dtype=torch.bool, device=_dev()), "proposal_boxes": torch.zeros(0, 4, device=_dev()),
             "mask_index": torch.zeros(0, dtype=torch.int64, device=_dev()), "gt_scores": torch.zeros(0, device=_dev())}]
    logits = head.layers(x)
    assert tuple(logits.shape) == (0, 1, 28, 28) and logits.dtype == dtype and logits.requires_grad
    loss = head(x, inst)["loss_mask"]
    assert loss.requires_grad and float(loss.detach()) == 0.0
    loss.backward()
    assert tuple(x.grad.shape) == (0, C, 14, 14)
    for k, p in head.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and float(p.grad.abs().max()) == 0.0, k
    assert head.eval()(x.detach(), [{"pred_boxes": torch.zeros(0, 4, device=_dev())}])[0]["pred_masks"].shape == (0, 1, 28, 28)


# ---------------------------------------------------------------------------------------------------------------- 7. forward_mask
def test_forward_mask_is_foreground_pooler_head():
    from unmore_amd import mask_head, roi_pool, roi_sample
    dev, C = _dev(), 64
    rng = np.random.RandomState(5)
    g = torch.Generator().manual_seed(6)
    feats = [torch.randn(2, C, 16, 24, generator=g).to(dev).requires_grad_(True), torch.randn(2, C, 8, 12, generator=g).to(dev).requires_grad_(True)]
    props, tgts = [], []
    for G in (3, 2):
        masks = blob_masks(rng, 64, 96, G)
        boxes = tight_boxes(masks)
        near, _ = jittered_proposals(rng, masks, 6, jitter=0.05)
        far = np.stack([np.array([x, y, x + 6, y + 5], dtype=np.float32) for x, y in rng.uniform(0, 50, (4, 2))])
        pb = np.concatenate([near, far]).astype(np.float32)
        props.append({"proposal_boxes": torch.from_numpy(pb).to(dev), "objectness_logits": torch.from_numpy(rng.randn(len(pb)).astype(np.float32)).to(dev)})
        tgts.append({"gt_boxes": torch.from_numpy(boxes).to(dev), "gt_classes": torch.zeros(G, dtype=torch.int64, device=dev),
                     "gt_scores": torch.from_numpy(rng.uniform(0.1, 0.9, G).astype(np.float32)).to(dev), "gt_masks": torch.from_numpy(masks).to(dev)})
    samples = roi_sample.label_and_sample_proposals(props, tgts, batch_size_per_image=16, positive_fraction=0.5, seed=1)
    pooler = roi_pool.ROIPooler(14, [0.25, 0.125], sampling_ratio=0, canonical_box_size=32, canonical_level=3)
    head = _head(C, (C, C, C), torch.bfloat16, mc.make_params(C, (C, C, C), seed=12)).train()
    loss = mask_head.forward_mask(feats, samples, pooler, head)["loss_mask"]
    fg = roi_sample.foreground(samples)
    n_fg = sum(len(i["gt_classes"]) for i in fg)
    assert n_fg >= 5 and n_fg < sum(len(i["gt_classes"]) for i in samples)
    by_hand = head(pooler(feats, [i["proposal_boxes"] for i in fg]), fg)["loss_mask"]
    assert float(loss.detach()) > 0 and torch.equal(loss.detach(), by_hand.detach())
    loss.backward()
    assert all(f.grad is not None and bool(torch.isfinite(f.grad).all()) and float(f.grad.abs().max()) > 0 for f in feats)
    assert torch.equal(mask_head.forward_mask({"p2": feats[0], "p3": feats[1]}, samples, pooler, head)["loss_mask"].detach(), loss.detach())
    head.eval()
    dets = [{"pred_boxes": p["proposal_boxes"][:7]} for p in props] + []
    dets[1] = {"pred_boxes": props[1]["proposal_boxes"][:0]}                              # an image without detections
    out = mask_head.forward_mask(feats, dets, pooler, head)
    assert out is dets and [tuple(d["pred_masks"].shape) for d in out] == [(7, 1, 28, 28), (0, 1, 28, 28)]


# ---------------------------------------------------------------------------------------------------------------- 8. stale weight copies
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_a_changed_parameter_reaches_the_next_call(name):
    dtype, C = DTYPES[name], 64
    dims = (C, C, C)
    head = _head(C, dims, dtype, mc.make_params(C, dims, seed=30)).train()
    x = mc.make_features(3, C, 7, seed=31).cuda()

    def fresh():
        return _head(C, dims, dtype, {k: v.detach().cpu() for k, v in head.state_dict().items()}).layers(x).detach()

    first = head.layers(x)
    assert torch.equal(first.detach(), head.layers(x).detach())                         # the cached copies, unchanged
    opt = torch.optim.SGD(head.parameters(), lr=0.05)
    first.backward(mc.make_dlogits(3, 7, 32).to(dtype).cuda())
    opt.step()
    second = head.layers(x).detach()
    assert not torch.equal(second, first.detach()) and torch.equal(second, fresh())
    with torch.no_grad():
        head.deconv.weight.mul_(1.5)
        head.mask_fcn1.bias.add_(0.25)
        head.predictor.weight.neg_()
    third = head.layers(x).detach()
    assert not torch.equal(third, second) and torch.equal(third, fresh())
    # another compute type is another set of copies
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    head.compute_dtype = other
    assert head.layers(x).dtype == other
    head.compute_dtype = dtype
    assert torch.equal(head.layers(x).detach(), third)
