"""unmore_amd.rpn_head on the device against the float64 restatement (tests/rpn_head_common.py).

Bounds.  The predictors sum in float32 on the matrix cores, whose internal order and rounding the ISA does not state: an output, a sum of
n = C + 1 terms, is held to 4 n 2^-24 sum |terms| (one ulp per addition, any order), plus 2^-8 |ref| for a bfloat16 store.  G is the n = 5A
bound plus one rounding to the compute type, exactly 0 where T <= 0; dWo, dWd, dbo, dbd are sums over the M rows: 4 M 2^-24 sum |terms|.
csrc/rpn_head.hip documents that a bfloat16 kernel rounds float32 incoming gradients to bfloat16 for the products of G and dW: those two
bounds get 2^-8 sum |terms| more in that case, and nothing else does.  The reference reads the predictor weights as the device does:
rounded to the compute type.  The convolution launches are held to the project's GEMM tolerance (gemm_forms_common.tol) against the
float64 layer applied to the device's OWN stored input.  End to end, the device's gradient error against float64 (e_dev) is held against
the error of the same chain in torch on the CPU in the compute type (e_ref): e_dev <= 2 e_ref + tol.atol max|ref|."""
import types

import numpy as np
import pytest
import torch

import rpn_head_common as hc
import rpn_loss_common as LC
from gemm_forms_common import tol
from mask_head_common import round_to
from test_rpn_gpu import _check_layers, _run

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
WKEYS = ("objectness_logits.weight", "objectness_logits.bias", "anchor_deltas.weight", "anchor_deltas.bias")


def _dev():
    return torch.device("cuda", 0)


def _ratio(err, allow):
    return float((err / allow.clamp_min(1e-300)).max()) if err.numel() else 0.0


def _close(x, ref, dtype, what):
    """x within tol(dtype) of ref everywhere; prints the largest error against its allowance"""
    t = tol(dtype)
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    assert x.shape == ref.shape, (what, x.shape, ref.shape)
    err, allow = (x - ref).abs(), t["atol"] + t["rtol"] * ref.abs()
    worst = _ratio(err, allow)
    print(f"{what}: max |err| {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e}, worst err / allowance {worst:.3f}")
    assert bool(torch.isfinite(x).all()) and worst <= 1.0, what


def _weights(sd, dtype):
    """the predictor weights as the device reads them (rounded to the compute type), the biases as they are; float64"""
    return [sd[k].to(dtype).double() if k.endswith("weight") else sd[k].double() for k in WKEYS]


def _head(C, A, dtype, sd=None):
    from unmore_amd.rpn_head import StandardRPNHead
    h = StandardRPNHead(C, A, compute_dtype=dtype)
    if sd is not None:
        h.load_state_dict(sd, strict=True)
    return h.to(_dev())


# ---------------------------------------------------------------------------------------------------------------- 1. the kernels alone
class Tail:
    """one shape and type: the inputs and every output of both kernels (twice), on the host"""

    def __init__(self, N, C, A, sizes, dtype):
        from unmore_amd import rpn_head
        self.N, self.C, self.A, self.sizes, self.dtype = N, C, A, list(sizes), dtype
        self.M = sum(N * h * w for h, w in sizes)
        self.T = hc.make_hidden(N, C, sizes, seed=100 + N + C).to(dtype)
        self.sd = hc.make_params(C, A, seed=C + A)
        self.dlog, self.ddel = hc.make_grad_maps(N, A, sizes, seed=9)
        dev = _dev()
        t = self.T.to(dev)
        w = [self.sd[k].to(dev) for k in WKEYS]
        self.out = {}
        for rep in (0, 1):
            for out_f32 in (False, True):
                lg, dl = rpn_head.predict(t, self.sizes, N, *w, out_f32=out_f32)
                self.out[("fwd", out_f32, rep)] = [x.cpu() for x in lg + dl]
            for g_f32 in ((True,) if dtype == torch.float32 else (False, True)):
                gd = torch.float32 if g_f32 else dtype
                tt = t.clone()
                G, dwo, dbo, dwd, dbd = rpn_head.predict_bwd(tt, self.sizes, N, [g.to(gd).to(dev) for g in self.dlog],
                                                             [g.to(gd).to(dev) for g in self.ddel], w[0], w[2])
                assert G.data_ptr() == tt.data_ptr()
                self.out[("bwd", g_f32, rep)] = [x.cpu() for x in (G, dwo, dbo, dwd, dbd)]
        assert torch.equal(t.cpu().view(torch.uint8), self.T.view(torch.uint8))         # predict only reads T


@pytest.fixture(scope="module")
def tails():
    cache = {}

    def get(shape, name):
        if (shape, name) not in cache:
            cache[(shape, name)] = Tail(*shape, DTYPES[name])
        return cache[(shape, name)]
    return get


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", hc.TAIL_SHAPES)
def test_predict_within_the_float32_sum_bound(tails, shape, name):
    t = tails(shape, name)
    w = _weights(t.sd, t.dtype)
    ref = hc.predict64(t.T, t.N, t.sizes, *w)
    scale = hc.predict_abs64(t.T, t.N, t.sizes, *w)
    for out_f32 in (False, True):
        got = t.out[("fwd", out_f32, 0)]
        odt = torch.float32 if out_f32 else t.dtype
        worst = 0.0
        for g, r, s in zip(got, ref[0] + ref[1], scale[0] + scale[1]):
            assert g.dtype == odt and g.shape == r.shape and g.is_contiguous() and bool(torch.isfinite(g).all())
            worst = max(worst, _ratio((g.double() - r).abs(), hc.out_allowance(t.C, s, r, odt)))
        print(f"{shape} {name} out_f32={out_f32}: worst err / allowance {worst:.4f}")
        assert worst <= 1.0
    flat = torch.cat([r.reshape(-1) for r in ref[0] + ref[1]])
    assert float(flat.min()) < 0 < float(flat.max())


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", hc.TAIL_SHAPES)
def test_predict_bwd_within_its_bounds_and_zero_under_the_mask(tails, shape, name):
    t = tails(shape, name)
    w = _weights(t.sd, t.dtype)
    for g_f32 in ((True,) if t.dtype == torch.float32 else (False, True)):
        gd = torch.float32 if g_f32 else t.dtype
        dlog, ddel = [g.to(gd) for g in t.dlog], [g.to(gd) for g in t.ddel]
        rounded = g_f32 and t.dtype == torch.bfloat16                                   # the documented rounding of float32 gradients
        G, dwo, dbo, dwd, dbd = t.out[("bwd", g_f32, 0)]
        ref = hc.predict_bwd64(t.T, t.N, t.sizes, dlog, ddel, w[0], w[2])
        sc = hc.predict_bwd_abs64(t.T, t.N, t.sizes, dlog, ddel, w[0], w[2])
        assert G.dtype == t.dtype and tuple(G.shape) == (t.M, t.C) and bool(torch.isfinite(G).all())
        assert bool((G[t.T <= 0] == 0).all())
        zero = float((G == 0).double().mean())
        rg = _ratio((G.double() - ref[0]).abs(), hc.g_allowance(t.A, sc[0], ref[0], t.dtype, rounded))
        rw = max(_ratio((got.double().reshape(r.shape) - r).abs(), hc.w_allowance(t.M, s, rounded))
                 for got, r, s in ((dwo, ref[1], sc[1]), (dwd, ref[3], sc[3])))
        rb = max(_ratio((got.double() - r).abs(), hc.w_allowance(t.M, s, False)) for got, r, s in ((dbo, ref[2], sc[2]), (dbd, ref[4], sc[4])))
        print(f"{shape} {name} grads_f32={g_f32}: worst err / allowance G {rg:.4f}, dW {rw:.4f}, db {rb:.4f}; zero fraction of G {zero:.3f}")
        assert all(x.dtype == torch.float32 for x in (dwo, dbo, dwd, dbd))
        assert tuple(dwo.shape) == (t.A, t.C) and tuple(dwd.shape) == (4 * t.A, t.C) and tuple(dbo.shape) == (t.A,) and tuple(dbd.shape) == (4 * t.A,)
        assert rg <= 1.0 and rw <= 1.0 and rb <= 1.0 and 0.3 < zero < 0.7


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", hc.TAIL_SHAPES)
def test_kernels_give_the_same_bytes_twice(tails, shape, name):
    t = tails(shape, name)
    for key, v in t.out.items():
        if key[-1] != 0:
            continue
        for a, b in zip(v, t.out[key[:-1] + (1,)]):
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), key


def test_entry_points_refuse_bad_arguments_without_a_launch():
    import ctypes
    from unmore_amd import _lib as L
    lib = L.lib()
    dev = _dev()
    T = torch.zeros(2 * 12, 64, dtype=torch.bfloat16, device=dev)
    lg, dl = torch.zeros(2, 3, 3, 4, dtype=torch.bfloat16, device=dev), torch.zeros(2, 12, 3, 4, dtype=torch.bfloat16, device=dev)
    wo, bo, wd, bd = torch.zeros(3, 64, device=dev), torch.zeros(3, device=dev), torch.zeros(12, 64, device=dev), torch.zeros(12, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    INVALID, UNSUPPORTED = -1, -2

    def table(n=1, H=3, W=4, a=lg.data_ptr(), b=dl.data_ptr()):
        tab = (ctypes.c_int64 * (4 * n))()
        for k in range(n):
            tab[4 * k:4 * k + 4] = [H, W, a, b]
        return tab

    def fwd(T_=p(T), tab=None, n=1, N=2, C=64, A=3, wo_=p(wo), bo_=p(bo), dtype=L.BF16):
        return lib.umr_rpn_head_predict(T_, table() if tab is None else tab, n, N, C, A, wo_, bo_, p(wd), p(bd), dtype, 0, None)

    def bwd(T_=p(T), tab=None, n=1, N=2, C=64, A=3, wo_=p(wo), dwo_=p(wo), dtype=L.BF16, ws_=p(ws), nbytes=1 << 16, phases=3):
        return lib.umr_rpn_head_predict_bwd(T_, table() if tab is None else tab, n, N, C, A, 0, wo_, p(wd), dwo_, p(bo), p(wd), p(bd), ws_,
                                            nbytes, dtype, phases, None)

    assert fwd() == 0 and bwd() == 0
    for call in (fwd, bwd):
        assert call(C=96) == UNSUPPORTED and call(C=2048) == UNSUPPORTED and call(C=0) == UNSUPPORTED
        assert call(A=4) == UNSUPPORTED and call(A=0) == UNSUPPORTED
        assert call(tab=table(9), n=9) == UNSUPPORTED and call(n=0) == UNSUPPORTED
        assert call(T_=None) == INVALID and call(wo_=None) == INVALID and call(dtype=7) == INVALID and call(N=-1) == INVALID
        assert call(tab=table(H=0)) == INVALID and call(tab=table(a=0)) == INVALID and call(tab=None, N=1 << 31) == INVALID
        assert b"rpn_head" in lib.umr_last_error_string()
    assert fwd(bo_=None) == INVALID
    assert bwd(dwo_=None) == INVALID and bwd(ws_=None) == INVALID and bwd(nbytes=16) == INVALID
    assert bwd(phases=0) == INVALID and bwd(phases=4) == INVALID
    assert fwd(T_=None, N=0) == 0 and bwd(T_=None, N=0) == 0                               # no rows: a successful no-op
    assert lib.umr_rpn_head_workspace(24, 64, 3) == 16 * 65 * 4 and lib.umr_rpn_head_workspace(129, 256, 1) == 2 * 16 * 257 * 4
    assert lib.umr_rpn_head_workspace(1 << 30, 256, 3) == 512 * 16 * 257 * 4               # the grid is capped whatever the device
    assert lib.umr_rpn_head_workspace(10, 96, 3) == -1 and lib.umr_rpn_head_workspace(10, 64, 4) == -1 and lib.umr_rpn_head_workspace(-1, 64, 3) == -1
    torch.cuda.synchronize()
    assert float(wo.abs().max()) == 0 and float(T.float().abs().max()) == 0


# ---------------------------------------------------------------------------------------------------------------- 2. layer by layer
MODULE_SIZES = ((16, 24), (8, 12), (4, 6), (2, 3), (1, 2))


class Run:
    """one forward and backward of the module with its stored activations and gradients, on the host"""

    def __init__(self, name, channels_last=False):
        dtype = DTYPES[name]
        N, C, A = 2, 64, 3
        self.N, self.C, self.A, self.dtype, self.sizes = N, C, A, dtype, list(MODULE_SIZES)
        self.sd = hc.make_params(C, A, seed=17)
        head = _head(C, A, dtype, self.sd)
        self.feats = hc.make_features(N, C, self.sizes, seed=5)
        xs = [f.to(_dev()) for f in self.feats]
        if channels_last:
            xs = [x.to(dtype).contiguous(memory_format=torch.channels_last) for x in xs]
        xs = [x.requires_grad_(True) for x in xs]
        keep = {}
        logits, deltas = head(xs, _keep=keep)
        self.dlog, self.ddel = [g.to(dtype) for g in hc.make_grad_maps(N, A, self.sizes, seed=11)[0]], \
                               [g.to(dtype) for g in hc.make_grad_maps(N, A, self.sizes, seed=11)[1]]
        torch.autograd.backward(logits + deltas, [g.to(_dev()) for g in self.dlog + self.ddel])
        self.logits, self.deltas = [t.detach().cpu() for t in logits], [t.detach().cpu() for t in deltas]
        self.x = [a.cpu() for a in keep["x"]]                                            # NHWC, in the compute type
        self.T = keep["T"].cpu()
        self.first = keep["first"]
        self.kept = {k: ([None if t is None else t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in keep["grads"].items()}
        self.gx = [x.grad.cpu() for x in xs]
        self.grads = {k: p.grad.cpu() for k, p in head.named_parameters()}


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name, channels_last=False):
        if (name, channels_last) not in cache:
            cache[(name, channels_last)] = Run(name, channels_last)
        return cache[(name, channels_last)]
    return get


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_module_forward_layer_by_layer(runs, name):
    r = runs(name)
    N, C, A = r.N, r.C, r.A
    cw, cb = r.sd["conv.weight"].to(r.dtype).double(), r.sd["conv.bias"].double()
    at = 0
    for k, (h, w) in enumerate(r.sizes):
        assert tuple(r.x[k].shape) == (N, h, w, C) and r.x[k].dtype == r.dtype
        assert torch.equal(r.x[k], hc.nhwc(r.feats[k]).to(r.dtype))                     # NCHW -> NHWC and the cast, exactly
        ref = hc.nhwc(hc.conv3_relu64(hc.nchw(r.x[k].double()), cw, cb)).reshape(-1, C)
        assert r.first[k] == at
        _close(r.T[at:at + N * h * w], ref, r.dtype, f"{name} conv level {k}")
        at += N * h * w
    assert at == r.T.shape[0] and 0.2 < float((r.T == 0).double().mean()) < 0.8
    wts = _weights(r.sd, r.dtype)
    ref = hc.predict64(r.T, N, r.sizes, *wts)
    scale = hc.predict_abs64(r.T, N, r.sizes, *wts)
    worst = max(_ratio((g.double() - rr).abs(), hc.out_allowance(C, s, rr, r.dtype))
                for g, rr, s in zip(r.logits + r.deltas, ref[0] + ref[1], scale[0] + scale[1]))
    print(f"{name} predictors on the module's own hidden map: worst err / allowance {worst:.4f}")
    assert worst <= 1.0 and all(g.dtype == r.dtype and g.is_contiguous() for g in r.logits + r.deltas)
    assert [tuple(g.shape) for g in r.logits] == [(N, A, h, w) for h, w in r.sizes]
    assert [tuple(g.shape) for g in r.deltas] == [(N, 4 * A, h, w) for h, w in r.sizes]


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_module_backward_layer_by_layer(runs, name):
    r = runs(name)
    N, C, A, M = r.N, r.C, r.A, r.T.shape[0]
    wts = _weights(r.sd, r.dtype)
    assert all(torch.equal(a, b) for a, b in zip(r.kept["dlogits"] + r.kept["ddeltas"], r.dlog + r.ddel))
    ref = hc.predict_bwd64(r.T, N, r.sizes, r.dlog, r.ddel, wts[0], wts[2])
    sc = hc.predict_bwd_abs64(r.T, N, r.sizes, r.dlog, r.ddel, wts[0], wts[2])
    G = r.kept["G"]
    assert bool((G[r.T <= 0] == 0).all())
    rg = _ratio((G.double() - ref[0]).abs(), hc.g_allowance(A, sc[0], ref[0], r.dtype, False))
    got = [r.grads[k] for k in WKEYS]
    rw = max(_ratio((got[i].double().reshape(ref[j].shape) - ref[j]).abs(), hc.w_allowance(M, sc[j], False)) for i, j in ((0, 1), (2, 3)))
    rb = max(_ratio((got[i].double() - ref[j]).abs(), hc.w_allowance(M, sc[j], False)) for i, j in ((1, 2), (3, 4)))
    print(f"{name} predictors' backward in the module: worst err / allowance G {rg:.4f}, dW {rw:.4f}, db {rb:.4f}")
    assert rg <= 1.0 and rw <= 1.0 and rb <= 1.0
    # the convolution's adjoint on the device's own G and stored inputs; its weight gradient is accumulated over the five levels
    cw = r.sd["conv.weight"].to(r.dtype).double()
    dW, db = torch.zeros_like(cw), torch.zeros(C, dtype=torch.float64)
    for k, (g, (h, w)) in enumerate(zip(hc.unstack_rows(G.double(), N, r.sizes), r.sizes)):
        dx, dw_l, db_l = hc.conv3_adjoint64(hc.nchw(r.x[k].double()), cw, g)
        _close(r.kept["dx"][k].reshape(N, h, w, C), hc.nhwc(dx), r.dtype, f"{name} conv data gradient level {k}")
        assert r.gx[k].dtype == torch.float32 and torch.equal(r.gx[k], hc.nchw(r.kept["dx"][k].reshape(N, h, w, C)).float())   # NHWC -> NCHW, exactly
        dW += dw_l
        db += db_l
    _close(r.grads["conv.weight"], dW, r.dtype, f"{name} conv.weight over five levels")
    _close(r.grads["conv.bias"], db, r.dtype, f"{name} conv.bias over five levels")
    assert all(g.dtype == torch.float32 and g.shape == r.sd[k].shape for k, g in r.grads.items())


def test_channels_last_inputs_in_the_compute_type_give_equal_outputs(runs):
    a, b = runs("bf16"), runs("bf16", True)
    assert all(torch.equal(x, y) for x, y in zip(a.logits + a.deltas, b.logits + b.deltas))
    assert torch.equal(a.T, b.T) and all(torch.equal(x, y) for x, y in zip(a.x, b.x))
    assert all(torch.equal(a.grads[k], b.grads[k]) for k in a.grads)
    assert all(g.dtype == torch.bfloat16 and torch.equal(g.float(), h.to(torch.bfloat16).float()) for g, h in zip(b.gx, a.gx))


# ---------------------------------------------------------------------------------------------------------------- 3. through RPN
E2E = dict(N=2, C=64, A=3, image_sizes=[(64, 96), (60, 90)], strides=[4, 8, 16, 32, 64], sizes=[[32], [64], [128], [256], [512]],
           ratios=[0.5, 1.0, 2.0], B=64, seed=12345)


def _gt(seed=3, G=3):
    rng = np.random.RandomState(seed)
    out = []
    for h, w in E2E["image_sizes"]:
        side = rng.uniform(16, 48, G)
        x1, y1 = rng.uniform(0, w - side), rng.uniform(0, h - side)
        out.append(np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.6, 1.0, G)], axis=1).astype(np.float32).reshape(-1, 4))
    return out


def _rpn(dtype, sd, **kw):
    from unmore_amd import rpn
    from unmore_amd.rpn_head import RPN
    cells = rpn.cell_anchors(E2E["sizes"], E2E["ratios"])
    return RPN(_head(E2E["C"], E2E["A"], dtype, sd), cells, E2E["strides"], batch_size_per_image=E2E["B"], pre_nms_topk=(300, 200),
               post_nms_topk=(100, 50), **kw), cells


def _same_proposals(proposals, logits, deltas, cells_np, dtype, pre, post, **kw):
    """`proposals` are rpn.rpn_proposals' on these (widened) head outputs, bit for bit, and rpn_common's in test_rpn_gpu's layers"""
    got, cand, counters = _run(logits, deltas, cells_np, E2E["strides"], E2E["image_sizes"], dtype=dtype, nms_thresh=0.7, pre_nms_topk=pre,
                               post_nms_topk=post, **kw)
    for n, (b, s) in enumerate(proposals):
        assert np.array_equal(b.cpu().numpy().view(np.uint32), got[n][0].view(np.uint32)), n
        assert np.array_equal(s.cpu().numpy().view(np.uint32), got[n][1].view(np.uint32)), n
    _check_layers(got, cand, counters, logits, deltas, cells_np, E2E["strides"], E2E["image_sizes"], 0.7, pre, post)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_rpn_end_to_end(name):
    dtype = DTYPES[name]
    N, C, A = E2E["N"], E2E["C"], E2E["A"]
    sd = hc.make_params(C, A, seed=23)
    model, cells = _rpn(dtype, sd)
    model.train()
    head = model.rpn_head
    feats0 = hc.make_features(N, C, MODULE_SIZES, seed=6)
    feats = {f"p{k + 2}": f.to(_dev()).requires_grad_(True) for k, f in enumerate(feats0)}
    gts = _gt()
    items = [{"gt_boxes": torch.from_numpy(g).to(_dev())} for g in gts]
    images = types.SimpleNamespace(image_sizes=E2E["image_sizes"])
    captured = {}
    orig = head.forward

    def spy(features, **kw):
        lg, dl = orig(features, **kw)
        for t in lg + dl:
            t.retain_grad()
        captured["logits"], captured["deltas"] = lg, dl
        return lg, dl
    head.forward = spy
    proposals, losses = model(images, feats, items, seed=E2E["seed"])
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc"}
    (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward(retain_graph=True)     # kept: the second backward below must reach the head
    lg, dl = captured["logits"], captured["deltas"]
    out_np = [t.detach().float().cpu().numpy() for t in lg + dl]
    nl = len(lg)
    cells_np = [c.numpy() for c in cells]
    # the proposals are rpn_common's on the head's own outputs: bit for bit what rpn.rpn_proposals gives on them, which is held to the
    # restatement in test_rpn_gpu's three layers (a last-bit difference of expf must not cascade through the NMS)
    _same_proposals(proposals, out_np[:nl], out_np[nl:], cells_np, dtype, 300, 100, training=True)
    assert len(proposals) == N and all(not b.requires_grad and len(b) > 10 for b, _ in proposals)
    # the losses are rpn_loss_common's on the same outputs
    lab = LC.label_and_sample_np(cells_np, E2E["strides"], list(MODULE_SIZES), gts, E2E["image_sizes"], E2E["B"], 0.5, seed=E2E["seed"])
    samples = [(s["pos"], s["neg"], s["gt"]) for s in lab]
    want = LC.losses_np(out_np[:nl], out_np[nl:], samples, cells_np, E2E["strides"], gts, E2E["B"])
    assert sum(len(s[0]) for s in samples) >= 4
    for key, w in (("loss_rpn_cls", want[0]), ("loss_rpn_loc", want[1])):
        got = float(losses[key].detach())
        print(f"{name} {key}: {got:.8f}, restated {float(w):.8f}")
        assert losses[key].dtype == torch.float32 and abs(got - float(w)) <= 1e-5 * max(1.0, abs(float(w))), key
    # gradients: float64 and the compute-type chain on the CPU, both with the device's own incoming dlogits / ddeltas
    gin = [t.grad.detach().cpu() for t in lg + dl]
    assert all(g is not None for g in gin) and sum(int((g != 0).sum()) for g in gin) >= 2 * E2E["B"]

    def chain(to, post):
        leaves = {k: v.clone().to(to).requires_grad_(True) for k, v in sd.items()}
        xs = [f.clone().to(to).requires_grad_(True) for f in feats0]
        params = {k: (post(v) if k.endswith("weight") else v) for k, v in leaves.items()}
        a, b = hc.head_chain([post(x) for x in xs], params, post)
        torch.autograd.backward(a + b, [g.to(to) for g in gin])
        return {**{k: v.grad for k, v in leaves.items()}, **{f"x{k}": x.grad for k, x in enumerate(xs)}}

    g64 = chain(torch.float64, lambda t: t)
    gref = chain(torch.float32, lambda t: round_to(t, dtype))
    gdev = {**{k: p.grad.cpu() for k, p in head.named_parameters()}, **{f"x{k}": f.grad.cpu() for k, f in enumerate(feats.values())}}
    t = tol(dtype)
    worst = 0.0
    for k in sorted(g64):
        r64 = g64[k]
        e_dev, e_ref = float((gdev[k].double() - r64).abs().max()), float((gref[k].double() - r64).abs().max())
        allow = 2 * e_ref + t["atol"] * float(r64.abs().max())
        worst = max(worst, e_dev / allow)
        print(f"{name} {k}: e_dev {e_dev:.3e}, e_ref {e_ref:.3e}, max |ref| {float(r64.abs().max()):.3e}, e_dev / allowance {e_dev / allow:.3f}")
    print(f"{name}: worst e_dev / allowance {worst:.3f}")
    for k in sorted(g64):
        r64 = g64[k]
        e_dev, e_ref = float((gdev[k].double() - r64).abs().max()), float((gref[k].double() - r64).abs().max())
        assert gdev[k].dtype == torch.float32 and e_dev <= 2 * e_ref + t["atol"] * float(r64.abs().max()), k
    # a second backward through the same forward
    with pytest.raises(RuntimeError, match="once per forward"):
        torch.autograd.backward(lg + dl, [torch.zeros_like(x) for x in lg + dl])
    # eval mode: the inference top-k, no losses, lists as well as dicts
    head.forward = orig
    model.eval()
    with torch.no_grad():
        props, none = model(E2E["image_sizes"], [f.detach() for f in feats.values()])
        lg2, dl2 = head([f.detach() for f in feats.values()])
    assert none == {} and len(props) == N and all(len(p[0]) <= 50 for p in props)
    _same_proposals(props, [x.float().cpu().numpy() for x in lg2], [x.float().cpu().numpy() for x in dl2], cells_np, dtype, 200, 50)
    boxes, scores, counts = model(E2E["image_sizes"], list(feats.values()), padded=True)[0]
    assert tuple(boxes.shape) == (N, 50, 4) and counts.tolist() == [len(p[0]) for p in props]


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_a_changed_parameter_reaches_the_next_call_and_empty_inputs_run(name):
    dtype = DTYPES[name]
    N, C, A = E2E["N"], E2E["C"], E2E["A"]
    model, _ = _rpn(dtype, hc.make_params(C, A, seed=31))
    model.train()
    head = model.rpn_head
    feats = [f.to(_dev()) for f in hc.make_features(N, C, MODULE_SIZES, seed=8)]

    def fresh():
        h = _head(C, A, dtype, {k: v.detach().cpu() for k, v in head.state_dict().items()})
        return torch.cat([t.detach().reshape(-1) for t in sum(h(feats), [])])

    def now():
        return torch.cat([t.detach().reshape(-1) for t in sum(head(feats), [])])
    first = now()
    assert torch.equal(first, now())                                                    # the cached copies, unchanged
    # empty ground truths: every sampled anchor is a negative, the localisation loss is 0 and both have gradients
    empty = [{"gt_boxes": torch.zeros(0, 4, device=_dev())} for _ in range(N)]
    _, losses = model(E2E["image_sizes"], feats, empty, seed=1)
    assert float(losses["loss_rpn_loc"].detach()) == 0.0 and float(losses["loss_rpn_cls"].detach()) > 0
    opt = torch.optim.SGD(head.parameters(), lr=0.5)
    (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in head.parameters())
    opt.step()
    second = now()
    assert not torch.equal(second, first) and torch.equal(second, fresh())
    with torch.no_grad():
        head.conv.weight.mul_(1.5)
        head.objectness_logits.bias.add_(0.25)
        head.anchor_deltas.weight.neg_()
    third = now()
    assert not torch.equal(third, second) and torch.equal(third, fresh())
    # a level without positions, and no images: empty outputs that are attached to the graph, zero gradients
    x0 = torch.zeros(N, C, 0, 5, device=_dev(), requires_grad=True)
    x1 = feats[3].clone().requires_grad_(True)
    lg, dl = head([x0, x1])
    assert tuple(lg[0].shape) == (N, A, 0, 5) and tuple(dl[0].shape) == (N, 4 * A, 0, 5) and lg[0].requires_grad
    (lg[0].sum() + dl[1].float().sum()).backward()
    assert tuple(x0.grad.shape) == (N, C, 0, 5) and float(x1.grad.abs().max()) > 0
    head.zero_grad()
    xe = torch.zeros(0, C, 4, 4, device=_dev(), requires_grad=True)
    lg, dl = head([xe])
    assert tuple(lg[0].shape) == (0, A, 4, 4) and lg[0].requires_grad
    (lg[0].sum() + dl[0].sum()).backward()
    assert tuple(xe.grad.shape) == (0, C, 4, 4)
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in head.parameters())
