"""Existence-classifier training on the MI355X: the new kernels (csrc/clf_train.hip) against torch on the CPU, and
ClassifierTrainStep against the float64 restatement of the reference loop (tests/clf_train_common.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import classifier_oracle as CO
from unmore_amd.hashrng import uniform, uniform01

from clf_train_common import OracleTrainer, adam_first_step, forward_train, param_names

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_stats_and_apply(dtype):
    from unmore_amd import ops
    dev = _dev()
    M, C = 3 * 17 * 13, 72
    z = _rnd((M, C), 1) * torch.linspace(0.1, 3.0, C) + _rnd((C,), 2)
    z[:, 5] = 1000.0 + 1.0 * _rnd((M,), 3)        # mean 10^3 x its standard deviation
    z = z.to(dtype)
    zd = z.to(dev)
    rm, rv = _rnd((C,), 4, 0.1), _rnd((C,), 5).abs() + 0.5
    rm_d, rv_d = rm.to(dev), rv.to(dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    mean, rstd = ops.bn_train_stats(zd, rm_d, rv_d, nbt)
    z64 = z.double()
    mu, var = z64.mean(0), z64.var(0, unbiased=False)
    torch.testing.assert_close(mean.cpu().double(), mu, rtol=1e-6, atol=1e-5)
    var_got = 1.0 / rstd.cpu().double() ** 2 - 1e-5
    assert ((var_got - var).abs() / var).max().item() < 1e-4
    # running statistics: what nn.BatchNorm2d writes, to fp32 rounding
    want_rm = (0.9 * rm.double() + 0.1 * mu).float()
    want_rv = (0.9 * rv.double() + 0.1 * z64.var(0, unbiased=True)).float()
    torch.testing.assert_close(rm_d.cpu(), want_rm, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(rv_d.cpu(), want_rv, rtol=1e-5, atol=0)
    assert int(nbt) == 1
    # apply: bn + ReLU, bn + second bn + ReLU, bn + residual + ReLU
    g, b = _rnd((C,), 6).abs() + 0.5, _rnd((C,), 7)
    z2 = (_rnd((M, C), 8) * 2 + 1).to(dtype)
    g2, b2 = _rnd((C,), 9).abs() + 0.5, _rnd((C,), 10)
    m2, r2 = ops.bn_train_stats(z2.to(dev))
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)

    def bn_ref(t, gg, bb):
        return F.batch_norm(t.double(), None, None, gg.double(), bb.double(), True, 0.1, 1e-5)
    y = ops.bn_train_apply(zd, mean, rstd, g.to(dev), b.to(dev))
    torch.testing.assert_close(y.float().cpu().double(), bn_ref(z, g, b).clamp_min(0), **tol)
    y = ops.bn_train_apply(zd, mean, rstd, g.to(dev), b.to(dev), second=(z2.to(dev), m2, r2, g2.to(dev), b2.to(dev)))
    torch.testing.assert_close(y.float().cpu().double(), (bn_ref(z, g, b) + bn_ref(z2, g2, b2)).clamp_min(0), **tol)
    y = ops.bn_train_apply(zd, mean, rstd, g.to(dev), b.to(dev), residual=z2.to(dev))
    torch.testing.assert_close(y.float().cpu().double(), (bn_ref(z, g, b) + z2.double()).clamp_min(0), **tol)


@pytest.mark.parametrize("two", [False, True])
def test_bn_backward_matches_autograd(two):
    """relu(bn(z) [+ bn_d(z_d) | + residual]) backward vs autograd of F.batch_norm(training=True); dy given directly and as the
    avg-pool gradient broadcast over each image's pixels"""
    from unmore_amd import ops
    dev = _dev()
    B, H, W, C = 3, 5, 7, 64
    M = B * H * W
    z = _rnd((M, C), 11) * 1.5 + 0.3
    zd = _rnd((M, C), 12) * 0.7 - 0.2
    res = _rnd((M, C), 13)
    g, b, gd, bd = _rnd((C,), 14).abs() + 0.5, _rnd((C,), 15), _rnd((C,), 16).abs() + 0.5, _rnd((C,), 17)
    dpool = _rnd((B, C), 18)
    for pooled in (False, True):
        zt, zdt, gt, bt, gdt, bdt = (t.double().requires_grad_(True) for t in (z, zd, g, b, gd, bd))
        out = F.batch_norm(zt, None, None, gt, bt, True, 0.1, 1e-5)
        out = out + (F.batch_norm(zdt, None, None, gdt, bdt, True, 0.1, 1e-5) if two else res.double())
        y = out.clamp_min(0)
        if pooled:
            (y.view(B, H * W, C).mean(1) * dpool.double()).sum().backward()
            src = dict(dpool=dpool.to(dev), rows_per_batch=H * W, pool_scale=1.0 / (H * W))
        else:
            dy = _rnd((M, C), 19)
            (y * dy.double()).sum().backward()
            src = dict(dy=dy.to(dev))
        m1, r1 = ops.bn_train_stats(z.to(dev))
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        br = [(z.to(dev), m1, r1, g.to(dev), dg, db)]
        if two:
            md, rd = ops.bn_train_stats(zd.to(dev))
            dgd, dbd = torch.empty(C, device=dev), torch.empty(C, device=dev)
            br.append((zd.to(dev), md, rd, gd.to(dev), dgd, dbd))
            dz, dzd = ops.bn_train_bwd(br, y=ops.bn_train_apply(z.to(dev), m1, r1, g.to(dev), b.to(dev), second=(zd.to(dev), md, rd,
                                                                                                                gd.to(dev), bd.to(dev))), **src)
        else:
            (dz,), gmask = ops.bn_train_bwd(br, y=ops.bn_train_apply(z.to(dev), m1, r1, g.to(dev), b.to(dev), residual=res.to(dev)),
                                           want_g=True, **src)
            torch.testing.assert_close(gmask.cpu().double(), _masked(y, src, B, H, W, C), rtol=1e-6, atol=1e-7)
        for got, want in ((dz, zt.grad), (dg, gt.grad), (db, bt.grad)) + (((dzd, zdt.grad), (dgd, gdt.grad), (dbd, bdt.grad)) if two else ()):
            scale = want.abs().max().item()
            assert (got.cpu().double() - want).abs().max().item() < 2e-5 * max(scale, 1e-3), (pooled, scale)


def _masked(y, src, B, H, W, C):
    """the gradient reaching the summed BN outputs (ReLU-masked), as the kernel's g_out"""
    if "dy" in src:
        g = src["dy"].cpu().double()
    else:
        g = (src["dpool"].cpu().double() * src["pool_scale"]).view(B, 1, C).expand(B, H * W, C).reshape(-1, C)
    return g * (y.detach() > 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_maxpool_backward_odd_extents_and_ties(dtype):
    from unmore_amd import ops
    dev = _dev()
    B, H, W, C = 2, 13, 11, 8
    x = _rnd((B, H, W, C), 21).abs()
    x[:, 2:5, 2:5, :3] = 0.75          # planted ties between positive values: the first maximum in scan order takes the gradient
    x[0, 6, 6, 4] = x[0, 6, 7, 4] = x[0, 7, 6, 4] = 3.0
    x = x.to(dtype)
    y = ops.maxpool3x3s2(x.to(dev))
    dy = _rnd(tuple(y.shape), 22).to(dtype)
    dx = ops.maxpool3x3s2_bwd(dy.to(dev), x.to(dev))
    xt = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(xt, 3, 2, 1).backward(dy.float().permute(0, 3, 1, 2))
    tol = dict(rtol=0, atol=0) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(dx.float().cpu(), xt.grad.permute(0, 2, 3, 1), **tol)


def test_stride2_scatter():
    from unmore_amd import ops
    dev = _dev()
    for (H, W) in ((9, 6), (8, 7)):
        dst = _rnd((2, H, W, 12), 31)
        src = _rnd((2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 12), 32)
        got = ops.stuff2_add(src.to(dev), dst.to(dev).clone())
        want = dst.clone()
        want[:, ::2, ::2, :] += src
        torch.testing.assert_close(got.cpu(), want, rtol=0, atol=0)


def test_bce_sigmoid_matches_torch_float32():
    from unmore_amd import ops
    dev = _dev()
    z = torch.cat([torch.linspace(-40, 40, 161), torch.tensor([0.0, 17.0, -17.0, 30.0, -30.0])])
    y = (torch.arange(z.numel()) % 2).float()
    zt = z.clone().requires_grad_(True)
    loss = F.binary_cross_entropy(torch.sigmoid(zt), y)
    loss.backward()
    got, dz = ops.bce_sigmoid(z.to(dev), y.to(dev))
    assert abs(got.item() - loss.item()) <= 1e-5 * max(1.0, abs(loss.item())), (got.item(), loss.item())
    torch.testing.assert_close(dz.cpu(), zt.grad, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------ the step
def _model(dtype=torch.float32):
    from unmore_amd.binary_classifier import Binary_Classifier
    net = Binary_Classifier(device="cuda:0", image_size=64, args=None, compute_dtype=dtype)
    net.load_state_dict(CO.hash_state("clf", uniform), strict=True)
    return net.to(_dev()).train()


def _batch(k, B, H, W):
    x = torch.from_numpy(uniform01(f"img:clf_train{k}", (B, 3, H, W))) * torch.linspace(0.5, 1.5, B).view(B, 1, 1, 1)
    y = torch.tensor([(i + k) % 2 for i in range(B)], dtype=torch.float32).view(B, 1)
    return x, y


def _flat_state(step):
    return step.flat_p.clone(), [b.clone() for b in step.net.buffers()]


@pytest.mark.parametrize("B,H,W,nsteps", [(4, 64, 64, 3), (2, 90, 70, 1)])
def test_step_matches_float64_reference_loop(B, H, W, nsteps):
    from unmore_amd import ClassifierTrainStep
    dev = _dev()
    net = _model()
    step = ClassifierTrainStep(net, lr=1e-3, lr_milestones=(2,), lr_gamma=0.1).set_graph_mode("off")
    orc = OracleTrainer(CO.hash_state("clf", uniform), lr=1e-3, milestones=(2,), gamma=0.1)
    named0 = {n: p.detach().clone() for n, p in net.named_parameters()}
    step.keep_activations = True
    for k in range(nsteps):
        x, y = _batch(k, B, H, W)
        before = {n: v.detach().cpu().clone() for n, v in net.state_dict().items()}
        w_m_v = (step.flat_p.clone(), step.m.clone(), step.v.clone())
        loss = step.step(x.to(dev), y.to(dev)).item()
        # gradients and losses are compared on the HIP path's linear piece: its ReLU decisions imposed on the float64 oracle, which
        # may differ from float64's own only within rounding of a kink (with batch statistics one such element moves the gradient
        # of its whole channel by up to ~10 % of the tensor's largest entry: measured at 64^2, B=4)
        masks = [a.permute(0, 3, 1, 2).cpu() > 0 for a in step.activations]
        flips = []
        loss_o, g_o = orc.step(x, y, masks if k == 0 else None, flips)
        if k == 0:
            assert len(flips) == 49 and max(f[1] for f in flips) < 1e-5, flips
            assert abs(loss - loss_o) < 1e-4, (loss, loss_o)
            G = step.grads()
            worst = max(((G[n].cpu().double() - g_o[n]).abs().max() / g_o[n].abs().max().clamp_min(1e-30)).item() for n in param_names())
            assert worst < 1e-3, worst
            sd, sdo = net.state_dict(), orc.state_dict()
            for n in sdo:
                if n.endswith(("running_mean", "running_var")):
                    torch.testing.assert_close(sd[n].cpu().double(), sdo[n], rtol=1e-4, atol=1e-6)
                elif n.endswith("num_batches_tracked"):
                    assert int(sd[n]) == 1, n
            # the step-1 weights are w0 - Adam(step.grads()), recomputed on the host
            for n, p in net.named_parameters():
                want = adam_first_step(named0[n].cpu(), G[n].cpu(), 1e-3)
                assert (p.detach().cpu().double() - want).abs().max().item() < 1e-6, n
        else:
            # this step's optimizer update, recomputed in float64 from the moments, weights and gradients the HIP step saw: Adam at
            # step k + 1 (its bias corrections) with the MultiStepLR rate of that step (1e-3 for step 2, 1e-4 after the milestone)
            # (the betas and 1 - beta as the f32 scalars of the library's Adam, umr_adam_step_hyper: 1 - 0.999f is 0.001 (1 - 1.3e-5))
            t, lr_t = k + 1, (1e-3 if k + 1 <= 2 else 1e-4)
            b1, b2 = np.float32(0.9), np.float32(0.999)
            c1, c2 = float(np.float32(1) - b1), float(np.float32(1) - b2)
            b1, b2 = float(b1), float(b2)
            w, m, v = (a.double() for a in w_m_v)
            g = step.flat_g.double()
            m = b1 * m + c1 * g
            v = b2 * v + c2 * g * g
            want = w - lr_t * (m / (1 - 0.9 ** t)) / ((v / (1 - 0.999 ** t)).sqrt() + 1e-8)
            assert (step.flat_p.double() - want).abs().max().item() < 1e-6, k
            assert (step.m.double() - m).abs().max().item() <= 1e-6 * m.abs().max().item(), k
            assert (step.v.double() - v).abs().max().item() <= 1e-6 * v.abs().max().item(), k
            # this step's loss from the weights the HIP steps produced (the packed copies were refreshed, the schedule advanced) ...
            own = F.binary_cross_entropy(torch.sigmoid(forward_train({n: (v.double() if v.is_floating_point() else v) for n, v in before.items()},
                                                                     x.double(), masks)), y.double())
            assert abs(loss - own.item()) < 1e-4 * max(1.0, abs(own.item())), (k, loss, own.item())
            # ... and from the float64 loop's own trajectory.  Adam's first update moves every weight by ~lr * sign(g): the 91 of
            # 25.6 M gradient entries whose sign is decided by rounding move 2e-3 apart, and the lr-1e-3 step 2 lands on a steep
            # part of the loss (6.2 from 0.80 at step 1), so step 3 differs by 9.1e-3 (measured; 2e-3 holds for step 2).  The step-3
            # bar is therefore 2e-2; steps 2 and 3 themselves are pinned by the two checks above.
            assert abs(loss - loss_o) < (2e-3 if k == 1 else 2e-2) * max(1.0, abs(loss_o)), (k, loss, loss_o)
    step.keep_activations = False
    assert step.iter == nsteps and abs(step.current_lr() - (1e-4 if nsteps >= 2 else 1e-3)) < 1e-12
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == CO.state_dict_spec()


@pytest.mark.parametrize("mode,nsteps", [("off", 2), ("on", 4)])
def test_eval_forward_between_steps_sees_the_trained_state(mode, nsteps):
    """An eval() forward between training steps (validation during training) fills Binary_Classifier's fold cache, keyed on the
    parameters' (data_ptr, _version); the step's kernels rewrite parameters and running statistics in place without bumping
    _version, so only the step's own invalidation keeps the next eval forward from serving the folded weights of the step
    before.  With mode 'on', steps 3 and 4 are graph replays."""
    from unmore_amd import ClassifierTrainStep
    dev = _dev()
    net = _model()
    step = ClassifierTrainStep(net, lr=1e-3).set_graph_mode(mode)
    x_eval = torch.from_numpy(uniform01("img:clf_train_eval", (3, 3, 64, 64)))
    prev = None
    for k in range(nsteps):
        net.train()
        step.step(*(t.to(dev) for t in _batch(k, 4, 64, 64)))
        net.eval()
        with torch.no_grad():
            got = net(x_eval.to(dev)).cpu().double()       # (re)fills the fold cache from the state after step k + 1
        sd = {n: (v.cpu().double() if v.is_floating_point() else v.cpu()) for n, v in net.state_dict().items()}
        want = CO.forward(sd, x_eval.double())
        assert (got - want).abs().max().item() < 1e-4, k
        if prev is not None:
            # a stale cache would serve `prev` (the state one step back): it must be outside the tolerance above
            assert (prev - want).abs().max().item() > 2e-4, (k, (prev - want).abs().max().item())
        prev = want
    assert step.graph_replays == (2 if mode == "on" else 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_checkpoint_resume_is_bit_identical(dtype):
    from unmore_amd import ClassifierTrainStep
    from unmore_amd.binary_classifier import Binary_Classifier
    dev = _dev()
    batches = [tuple(t.to(dev) for t in _batch(k, 2, 64, 64)) for k in range(3)]
    net = _model(dtype)
    step = ClassifierTrainStep(net, lr=1e-3, lr_milestones=(2,), lr_gamma=0.1).set_graph_mode("off")
    losses = [step.step(*b).item() for b in batches[:2]]
    ckpt = {"model_state_dict": {k: v.clone() for k, v in net.state_dict().items()}, "optimizer_state_dict": step.optimizer_state_dict(),
            "iter": step.iter}
    loss3 = step.step(*batches[2]).item()
    final = {k: v.clone() for k, v in net.state_dict().items()}
    # the optimizer half is torch.optim.Adam's own format
    ref = Binary_Classifier(device="cpu", image_size=64, args=None)
    torch.optim.Adam(ref.parameters(), lr=1e-3).load_state_dict(
        {"state": {i: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in s.items()} for i, s in ckpt["optimizer_state_dict"]["state"].items()},
         "param_groups": ckpt["optimizer_state_dict"]["param_groups"]})
    net2 = Binary_Classifier(device="cuda:0", image_size=64, args=None, compute_dtype=dtype)
    net2.load_state_dict(ckpt["model_state_dict"], strict=True)
    net2 = net2.to(dev).train()
    step2 = ClassifierTrainStep(net2, lr=1e-3, lr_milestones=(2,), lr_gamma=0.1).set_graph_mode("off")
    step2.load_optimizer_state_dict(ckpt["optimizer_state_dict"], iteration=ckpt["iter"])
    step2.sync_from_model()
    assert step2.iter == 2 and len(losses) == 2
    assert step2.step(*batches[2]).item() == loss3
    for k, v in net2.state_dict().items():
        assert torch.equal(v, final[k]), k


def test_determinism_and_graph_replay_bit_identical():
    from unmore_amd import ClassifierTrainStep
    dev = _dev()
    batches = [tuple(t.to(dev) for t in _batch(k, 2, 64, 64)) for k in range(5)]
    runs = []
    for mode in ("off", "off", "on"):
        net = _model()
        step = ClassifierTrainStep(net, lr=1e-3).set_graph_mode(mode)
        losses = [step.step(*b).item() for b in batches]
        runs.append((losses, step.flat_p.clone(), [b.clone() for b in net.buffers()], step.graph_replays))
    assert runs[0][3] == 0 and runs[2][3] == 3        # steps 3..5 of the 'on' run are graph replays
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert torch.equal(other[1], runs[0][1])
        assert all(torch.equal(a, b) for a, b in zip(other[2], runs[0][2]))


def _ellipse_batch(k, B, S):
    from unmore_amd import synth
    masks = synth.ellipse_masks(B, S, S, seed=100 + k).astype(np.float32)
    x = uniform01(f"img:clf_ell{k}", (B, 3, S, S)) * 0.5
    y = (np.arange(B) % 2).astype(np.float32)
    x = x + (y[:, None, None, None] * masks[:, None]) * 0.5      # label 1: the image contains a filled ellipse
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y).view(B, 1)


def test_bf16_tracks_fp32_and_learns():
    from unmore_amd import ClassifierTrainStep
    dev = _dev()
    x, y = _batch(0, 4, 64, 64)
    orc = OracleTrainer(CO.hash_state("clf", uniform), lr=1e-3)
    loss_o, _ = orc.step(x, y)
    net = _model(torch.bfloat16)
    step = ClassifierTrainStep(net, lr=1e-3)
    loss0 = step.step(x.to(dev), y.to(dev)).item()
    # measured: 0.7924 vs 0.8037 (1.1e-2: bf16 storage of every activation); the bar leaves 4x margin
    print(f"bf16 first-step loss {loss0:.6f} vs float64 oracle {loss_o:.6f}")
    assert abs(loss0 - loss_o) < 0.05 * max(1.0, abs(loss_o)), (loss0, loss_o)
    losses = []
    for k in range(30):
        xb, yb = _ellipse_batch(k, 8, 64)
        losses.append(step.step(xb.to(dev), yb.to(dev)).item())
    first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
    # measured: 1.45 over steps 1-5, 0.0000 over steps 26-30; the bar asks for a 30 % drop
    print(f"bf16 ellipse task: mean loss of steps 1-5 {first:.4f}, of steps 26-30 {last:.4f}")
    assert np.isfinite(losses).all() and last < 0.7 * first, losses


def test_rejected_inputs_leave_state_untouched():
    from unmore_amd import ClassifierTrainStep
    dev = _dev()
    net = _model()
    step = ClassifierTrainStep(net, lr=1e-3)
    p0, b0 = _flat_state(step)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        step.step(torch.rand(1, 3, 32, 32, device=dev), torch.ones(1, 1, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        step.step(torch.rand(2, 3, 64, 64), torch.ones(2, 1))
    torch.cuda.synchronize()
    p1, b1 = _flat_state(step)
    assert step.iter == 0 and torch.equal(p0, p1) and all(torch.equal(a, b) for a, b in zip(b0, b1))
    step.step(torch.rand(2, 3, 32, 32, device=dev), torch.ones(2, 1, device=dev))    # B=2 at 32^2: two values per channel, accepted
    assert step.iter == 1
