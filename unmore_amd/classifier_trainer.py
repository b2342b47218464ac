"""Native training step for the existence classifier (reference: BinaryClassifierTrainer, train_objectness_net.py:540-743:
torchvision ResNet-50 -> Linear(1000, 1) -> sigmoid under BCELoss, Adam and a per-iteration MultiStepLR; stage 1.2 of
README.md:147-163, `--train_existence`).

`ClassifierTrainStep(model).step(images, labels)` replaces the reference loop body (:652-662) after `model.train()`: BatchNorm
normalises with the batch statistics and updates the running statistics (momentum 0.1, unbiased running variance,
num_batches_tracked + 1), the loss is BCELoss(mean) of the sigmoid of the head, and Adam updates all 163 parameter tensors.
Nothing runs on autograd or on PyTorch's kernels: the convolutions and Linear layers are umr_gemm_nt / umr_gemm_tn launches
(forward, data gradient, weight gradient), the BatchNorm statistics / normalisation / backward, the max-pool backward, the
stride-2 shortcut scatter and the loss are csrc/clf_train.hip, the optimizer is one umr_adam_step_hyper launch over a flat
buffer the parameters are re-homed into (trainer.rehome_params), followed by one umr_permute4_batched launch that refreshes
every packed weight copy.  Layout NHWC; activations are stored in the model's compute dtype (f32 or bf16), statistics,
gradients of parameters and the classifier tail (avg-pool, fc, head, loss) in f32.

The step never calls `Binary_Classifier.forward` (which keeps refusing training mode); after every step the module's
eval-mode fold cache is dropped, so an eval() forward sees the trained weights and running statistics."""
import torch

from . import graphs, ops
from .binary_classifier import _BN_EPS, _LAYERS
from .trainer import AdamState, rehome_params

_BN_MOMENTUM = 0.1
_STEM_LDK = 152       # 3 * 7 * 7 = 147 columns of the stem's im2col rows, padded to a multiple of 8


def _down2(n):
    return (n - 1) // 2 + 1


def smallest_bn_rows(B, H, W):
    """Values per channel the last BatchNorms (layer4) see: B * H5 * W5 after the stem conv, the max-pool and three stride-2 stages"""
    for _ in range(5):
        H, W = _down2(H), _down2(W)
    return B * H * W


class ClassifierTrainStep(AdamState):
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, lr_milestones=(), lr_gamma=1.0):
        self.net = model
        self.lr0, self.betas, self.eps = lr, tuple(betas), eps
        self.milestones, self.gamma = tuple(lr_milestones), lr_gamma
        self.iter = 0
        self.poisoned = None
        named = dict(model.named_parameters())
        dev = next(iter(named.values())).device
        if dev.type != "cuda":
            raise RuntimeError("unmore_amd.ClassifierTrainStep runs on the MI355X only (no CPU fallback); move the model to the GPU first")
        offs, off = {}, 0
        for n, p in named.items():      # model.parameters() order; every view 256-byte aligned
            offs[n] = off
            off += (p.numel() + 63) // 64 * 64
        self.flat_p, self.flat_g, self.m, self.v, self.G = rehome_params(named, offs, off, dev)
        self.P = dict(model.named_parameters())
        self._offs = offs
        self._hyper = torch.zeros(8, dtype=torch.float32, device=dev)
        self.graph_mode = graphs.DEFAULT_MODE
        self._graphs = {}           # (input shape, dtype, f32 mode, stream) -> eager-call count, then graphs.Captured
        self.graph_replays = 0
        rb = model.classifier_backbone
        self.blocks = [blk for li in range(4) for blk in getattr(rb, f"layer{li + 1}")]
        self.keep_activations = False   # tests: keep the post-ReLU maps of the last step (self.activations, NHWC, ReLU order)
        self.activations = None
        self._packs = None
        self._pack_packs(dev)

    # ---- packed (kernel-layout) weight copies, refreshed in place after every update
    def _pack_packs(self, dev):
        dt = self.net.compute_dtype
        recipes = []

        def lin(w):            # 1x1 conv [co, ci, 1, 1] -> [co, ci] (the parameter itself in f32)
            co, ci = w.shape[0], w.shape[1]
            if dt == torch.float32:
                return w.detach().view(co, ci)
            out = torch.empty((co, ci), dtype=dt, device=dev)
            recipes.append((w.detach(), out, (1, 1, co, ci), (0, 0, ci, 1), 0))
            return out

        def lin_t(w):          # 1x1 conv data gradient: [ci, co]
            co, ci = w.shape[0], w.shape[1]
            out = torch.empty((ci, co), dtype=dt, device=dev)
            recipes.append((w.detach(), out, (1, 1, ci, co), (0, 0, 1, ci), 0))
            return out

        def c3(w):             # [co, ci, 3, 3] -> [co][ky][kx][ci]
            co, ci = w.shape[0], w.shape[1]
            out = torch.empty((co, 9 * ci), dtype=dt, device=dev)
            recipes.append((w.detach(), out, (co, 3, 3, ci), (9 * ci, 3, 1, 9), 0))
            return out

        def c3_d(w):           # data gradient: [ci][2-ky][2-kx][co]
            co, ci = w.shape[0], w.shape[1]
            out = torch.empty((ci, 9 * co), dtype=dt, device=dev)
            recipes.append((w.detach(), out, (ci, 3, 3, co), (9, -3, -1, 9 * ci), 8))
            return out

        K = {"blocks": []}
        for blk in self.blocks:
            e = {"c1": lin(blk.conv1.weight), "c1_t": lin_t(blk.conv1.weight), "c2": c3(blk.conv2.weight), "c2_d": c3_d(blk.conv2.weight),
                 "c3": lin(blk.conv3.weight), "c3_t": lin_t(blk.conv3.weight)}
            if blk.downsample is not None:
                e["d"], e["d_t"] = lin(blk.downsample[0].weight), lin_t(blk.downsample[0].weight)
            K["blocks"].append(e)
        fc = self.net.classifier_backbone.fc
        K["fc_t"] = torch.empty((2048, 1000), dtype=torch.float32, device=dev)
        recipes.append((fc.weight.detach(), K["fc_t"], (1, 1, 2048, 1000), (0, 0, 1, 2048), 0))
        # the stem's rows padded to _STEM_LDK columns with zeros: umr_bn_fold with a unit scale (gamma 1, var 1, eps 0) and zero shift
        K["stem"] = torch.empty((64, _STEM_LDK), dtype=dt, device=dev)
        K["stem_b"] = torch.empty(64, dtype=torch.float32, device=dev)
        K["one"] = torch.ones(64, dtype=torch.float32, device=dev)
        K["zero"] = torch.zeros(64, dtype=torch.float32, device=dev)
        K["refresh"] = ops.permute4_batched(recipes)
        K["dtype"] = dt
        self._packs = K
        self._refresh_packs()

    def _refresh_packs(self):
        K = self._packs
        K["refresh"]()
        w = self.net.classifier_backbone.conv1.weight.detach().view(64, 147)
        ops.bn_fold(w, K["one"], K["zero"], K["zero"], K["one"], 0.0, _STEM_LDK, K["dtype"], w_out=K["stem"], b_out=K["stem_b"])

    # ---- one step: forward with batch statistics, loss, backward, Adam, weight-copy refresh
    def _stats(self, z, bn):
        return ops.bn_train_stats(z, bn.running_mean, bn.running_var, bn.num_batches_tracked, _BN_EPS, _BN_MOMENTUM)

    def _body(self, images, labels):
        K, G, dt = self._packs, self.G, self._packs["dtype"]
        rb = self.net.classifier_backbone
        head = self.net.binary_classification_head
        B = images.shape[0]
        dev = images.device
        # ---- forward
        cols, H1, W1 = ops.im2col_nchw(images, 7, 7, 2, 3, _STEM_LDK, dt)
        z0 = ops.gemm_nt(cols, K["stem"])
        st0 = self._stats(z0, rb.bn1)
        a0 = ops.bn_train_apply(z0, *st0, rb.bn1.weight.detach(), rb.bn1.bias.detach()).view(B, H1, W1, 64)
        h = ops.maxpool3x3s2(a0)
        saved = []
        acts = [a0]
        for blk, e in zip(self.blocks, K["blocks"]):
            _, H, W, C = h.shape
            s = blk.stride
            Ho, Wo = _down2(H) if s == 2 else H, _down2(W) if s == 2 else W
            x2d = h.view(-1, C)
            z1 = ops.gemm_nt(x2d, e["c1"])
            p = z1.shape[1]
            st1 = self._stats(z1, blk.bn1)
            a1 = ops.bn_train_apply(z1, *st1, blk.bn1.weight.detach(), blk.bn1.bias.detach())
            z2 = ops.gemm_nt(a1.view(B, H, W, p), e["c2"], conv=(2 if s == 2 else 1))
            st2 = self._stats(z2, blk.bn2)
            a2 = ops.bn_train_apply(z2, *st2, blk.bn2.weight.detach(), blk.bn2.bias.detach())
            z3 = ops.gemm_nt(a2, e["c3"])
            st3 = self._stats(z3, blk.bn3)
            sv = {"x": h, "z1": z1, "st1": st1, "a1": a1, "z2": z2, "st2": st2, "a2": a2, "z3": z3, "st3": st3, "hw": (H, W, Ho, Wo)}
            if blk.downsample is not None:
                xin = x2d
                if s == 2:   # 1x1 stride-2 conv = 1x1 conv of the subsampled map
                    xs = torch.empty((B, Ho, Wo, C), dtype=dt, device=dev)
                    ops.permute4(h, xs, (B, Ho, Wo, C), (H * W * C, 2 * W * C, 2 * C, 1))
                    xin = xs.view(-1, C)
                zd = ops.gemm_nt(xin, e["d"])
                bnd = blk.downsample[1]
                std = self._stats(zd, bnd)
                out = ops.bn_train_apply(z3, *st3, blk.bn3.weight.detach(), blk.bn3.bias.detach(),
                                         second=(zd, *std, bnd.weight.detach(), bnd.bias.detach()))
                sv.update(xin=xin, zd=zd, std=std)
            else:
                out = ops.bn_train_apply(z3, *st3, blk.bn3.weight.detach(), blk.bn3.bias.detach(), residual=x2d)
            sv["out"] = out
            saved.append(sv)
            if self.keep_activations:
                acts += [a1.view(B, H, W, p), a2.view(B, Ho, Wo, p), out.view(B, Ho, Wo, 4 * p)]
            h = out.view(B, Ho, Wo, 4 * p)
        _, H, W, C = h.shape
        HW = H * W
        pooled = ops.cast(ops.segsum(h, B, HW, C, HW * C, C, out_f32=True), torch.float32, scale=1.0 / HW)   # AdaptiveAvgPool2d(1)
        fc = rb.fc
        logits = ops.gemm_nt(pooled, fc.weight.detach(), fc.bias.detach())                  # [B, 1000] f32
        zhead = ops.gemm_nt(logits, head.weight.detach(), head.bias.detach(), out_f32=True)  # [B, 1] f32
        loss, dlogit = ops.bce_sigmoid(zhead, labels)
        self.activations = acts if self.keep_activations else None

        # ---- backward: head, fc
        nh = "binary_classification_head."
        ops.small_gemm(dlogit, logits, G[nh + "weight"], 1, 1000, B, (0, 1), (1000, 1), (0, 1))
        ops.segsum(dlogit, 1, B, 1, 0, 1, out=G[nh + "bias"].view(1, 1))
        dlogits = torch.empty((B, 1000), dtype=torch.float32, device=dev)
        ops.small_gemm(dlogit, head.weight.detach(), dlogits, B, 1000, 1, (1, 0), (0, 1), (1000, 1))
        nb = "classifier_backbone."
        ops.gemm_tn(dlogits, pooled, dW=G[nb + "fc.weight"], dbias=G[nb + "fc.bias"])
        dpooled = ops.gemm_nt(dlogits, K["fc_t"])                                            # [B, 2048] f32
        del dlogits

        # ---- backward: bottlenecks, last first; the last block's gradient is the avg-pool's, broadcast inside the BN kernels
        names = [f"{nb}layer{li + 1}.{bi}." for li, (_, blocks, _) in enumerate(_LAYERS) for bi in range(blocks)]
        src = {"dpool": dpooled, "rows_per_batch": HW, "pool_scale": 1.0 / HW}
        for blk, e, sv, pre in reversed(list(zip(self.blocks, K["blocks"], saved, names))):
            H, W, Ho, Wo = sv["hw"]
            x = sv["x"]
            C = x.shape[-1]
            p = sv["z1"].shape[1]
            s = blk.stride
            br = [(sv["z3"], *sv["st3"], blk.bn3.weight.detach(), G[pre + "bn3.weight"], G[pre + "bn3.bias"])]
            down = blk.downsample is not None
            if down:
                br.append((sv["zd"], *sv["std"], blk.downsample[1].weight.detach(), G[pre + "downsample.1.weight"], G[pre + "downsample.1.bias"]))
                dz3, dzd = ops.bn_train_bwd(br, y=sv["out"], **src)
            else:
                (dz3,), g = ops.bn_train_bwd(br, y=sv["out"], want_g=True, **src)
            ops.gemm_tn(dz3, sv["a2"], dW=G[pre + "conv3.weight"].view(4 * p, p))
            da2 = ops.gemm_nt(dz3, e["c3_t"])
            del dz3
            (dz2,) = ops.bn_train_bwd([(sv["z2"], *sv["st2"], blk.bn2.weight.detach(), G[pre + "bn2.weight"], G[pre + "bn2.bias"])], dy=da2,
                                      y=sv["a2"])
            del da2
            a1 = sv["a1"].view(B, H, W, p)
            dwp = ops.gemm_tn(dz2, a1, conv=(2 if s == 2 else 1))                              # [p][ky][kx][ci]
            ops.permute4(dwp, G[pre + "conv2.weight"], (p, p, 3, 3), (9 * p, 1, 3 * p, p))
            dz2 = dz2.view(B, Ho, Wo, p)
            if s == 2:
                dz2 = ops.zero_stuff2(dz2, H, W)
            da1 = ops.gemm_nt(dz2, e["c2_d"], conv=1)
            del dz2
            (dz1,) = ops.bn_train_bwd([(sv["z1"], *sv["st1"], blk.bn1.weight.detach(), G[pre + "bn1.weight"], G[pre + "bn1.bias"])], dy=da1,
                                      y=sv["a1"])
            del da1
            x2d = x.view(-1, C)
            ops.gemm_tn(dz1, x2d, dW=G[pre + "conv1.weight"].view(p, C))
            if down:
                ops.gemm_tn(dzd, sv["xin"], dW=G[pre + "downsample.0.weight"].view(4 * p, C))
                dxd = ops.gemm_nt(dzd, e["d_t"])
                if s == 2:
                    dx = ops.gemm_nt(dz1, e["c1_t"])
                    ops.stuff2_add(dxd.view(B, Ho, Wo, C), dx.view(B, H, W, C))
                else:
                    dx = ops.gemm_nt(dz1, e["c1_t"], aux=dxd)
                del dxd
            else:
                dx = ops.gemm_nt(dz1, e["c1_t"], aux=g)
            del dz1
            src = {"dy": dx}
            sv.clear()

        # ---- stem: max-pool backward, BN + ReLU backward, weight gradient over the im2col rows (no data gradient)
        da0 = ops.maxpool3x3s2_bwd(src["dy"].view(B, _down2(H1), _down2(W1), 64), a0)
        (dz0,) = ops.bn_train_bwd([(z0, *st0, rb.bn1.weight.detach(), G[nb + "bn1.weight"], G[nb + "bn1.bias"])], dy=da0.view(-1, 64),
                                  y=a0.view(-1, 64))
        dws = ops.gemm_tn(dz0, cols)                                                         # [64, _STEM_LDK]
        ops.permute4(dws, G[nb + "conv1.weight"], (1, 1, 64, 147), (0, 0, _STEM_LDK, 1))

        # ---- Adam over the flat buffer (scalars from device memory), then every packed copy
        ops.adam_step_hyper(self.flat_p, self.flat_g, self.m, self.v, self._hyper)
        self._refresh_packs()
        return (loss,)

    # ---- public interface (mirrors trainer.TrainStep)
    def set_graph_mode(self, mode):
        """'auto' (default; env UMR_GRAPHS): steps of small problems (B*H*W <= 2^20 pixels: the reference's recipe) are captured after
        two eager steps of the same shape as ONE single-stream HIP graph and replayed; larger ones run eagerly.  'on' captures any
        size, 'off' nothing."""
        assert mode in ("auto", "on", "off")
        self.graph_mode = mode
        self._graphs.clear()
        return self

    def step(self, images, class_labels):
        """One optimisation step on images [B, 3, H, W] (f32, [0, 1]) and class_labels [B, 1] (f32 in {0, 1}); returns the loss
        (device f32 [1])."""
        if not (images.is_cuda and class_labels.is_cuda):
            raise RuntimeError("unmore_amd.ClassifierTrainStep runs on the MI355X only (no CPU fallback); move images and labels to the GPU")
        if images.dim() != 4 or images.shape[1] != 3 or class_labels.numel() != images.shape[0]:
            raise ValueError(f"ClassifierTrainStep.step: images [B, 3, H, W] and labels [B, 1] expected, got {tuple(images.shape)} and "
                             f"{tuple(class_labels.shape)}")
        B, _, H, W = images.shape
        if smallest_bn_rows(B, H, W) <= 1:
            # torch's BatchNorm raises for this batch in training mode; refuse before anything is launched or updated
            raise ValueError(f"Expected more than 1 value per channel when training: a batch of {B} image(s) of {H}x{W} leaves "
                             f"{smallest_bn_rows(B, H, W)} value(s) per channel at the last BatchNorm layers")
        if self.poisoned is not None:
            raise RuntimeError("ClassifierTrainStep: an earlier step raised after part of its update was enqueued (" + self.poisoned +
                               "); reload a checkpoint (model.load_state_dict, load_optimizer_state_dict, sync_from_model) first")
        if self._packs["dtype"] != self.net.compute_dtype:
            self._graphs.clear()
            self._pack_packs(images.device)
        images = images.float().contiguous()
        labels = class_labels.reshape(-1).float().contiguous()
        it = self.iter + 1
        ops.adam_set_hyper(self._hyper, it, self.lr_of_step(it), self.betas[0], self.betas[1], self.eps)
        try:
            loss = self._launch_step(images, labels)
        except BaseException as e:
            self.poisoned = f"{type(e).__name__}: {e}"
            raise
        finally:
            self.net._packed = None    # Binary_Classifier's eval-mode fold cache: kernel writes do not bump tensor versions
        self.iter = it
        return loss

    def _launch_step(self, images, labels):
        B, _, H, W = images.shape
        if graphs.wanted(self.graph_mode, B * H * W):
            key = (tuple(images.shape), self._packs["dtype"], ops.get_f32_mode(), torch.cuda.current_stream(images.device).cuda_stream)
            outs = graphs.replay_or_capture(self._graphs, key, (images, labels), lambda: graphs.Captured(self._body, (images, labels)))
            if outs is not None:
                self.graph_replays += 1
                return outs[0].clone()
        return self._body(images, labels)[0]

    def evaluate(self, batches):
        """The reference's evaluate_classification (train_objectness_net.py:703-743) without its image dump: `batches` yields
        (images [B, 3, H, W], class_labels [B, 1]); the model runs in eval() mode under no_grad (Binary_Classifier.forward: running
        statistics folded into the convolutions), hits += ((pred > 0.5) == label).sum() accumulates on the device and is read
        once at the end.  Returns (hits, total); accuracy = hits / total is what the reference logs under the iteration.
        The model goes back into the mode it was in, also when a batch raises.  Nothing the step owns is touched: parameters,
        running statistics, Adam state, `iter` and the captured step graphs are as before."""
        was_training = self.net.training
        self.net.eval()
        hits, total = None, 0
        try:
            with torch.no_grad():
                for images, class_labels in batches:
                    if not (images.is_cuda and class_labels.is_cuda):
                        raise RuntimeError("unmore_amd.ClassifierTrainStep runs on the MI355X only (no CPU fallback); move images and labels "
                                           "to the GPU")
                    pred = self.net(images=images)                                                  # :716
                    n = ((pred > 0.5).to(class_labels.dtype) == class_labels.reshape(pred.shape)).sum()   # :717-719
                    hits = n if hits is None else hits + n
                    total += pred.shape[0]                                                          # :719
        finally:
            self.net.train(was_training)                                                            # :741
        return (int(hits.item()) if hits is not None else 0), total

    def grads(self):
        """{parameter name: gradient view} of the last step (views into the flat gradient buffer)"""
        return dict(self.G)

    def sync_from_model(self):
        """Call after model.load_state_dict(): the flat buffer is the parameters' storage, so loading writes through; the packed
        weight copies and the module's eval-mode fold cache are rebuilt from it."""
        self._refresh_packs()
        self.net._packed = None
