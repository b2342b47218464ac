"""Training-mode restatement of the existence classifier for the tests (no test file of its own: imported by test_clf_train_*.py).

What the reference loop does after `self.model.train()` (train_objectness_net.py:584-587,652-662): torchvision ResNet-50 with
BatchNorm on batch statistics (F.batch_norm(training=True), momentum 0.1, eps 1e-5), Linear(1000, 1), sigmoid, BCELoss(mean),
torch.optim.Adam over model.parameters(), MultiStepLR stepped per iteration -- built from oracle.classifier_oracle's key names and
hash_state, run on the CPU in float64 with torch's own implementations."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import classifier_oracle as CO

BN_MOMENTUM = 0.1


def param_names():
    """The 163 parameter names in model.parameters() order"""
    return [n for n, _ in CO.state_dict_spec() if not n.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def forward_train(sd, x, masks=None, flips=None, training=True):
    """[B,3,H,W] -> logits [B,1] (pre-sigmoid), BatchNorm in training mode; sd's running_mean / running_var are updated in place and
    its num_batches_tracked incremented, as nn.BatchNorm2d does.  training=False: the same graph with BatchNorm in eval form
    (running statistics, nothing updated) -- the eval oracle's forward.
    masks: the 49 ReLU decisions of another arithmetic path (NCHW bool, in ReLU order: stem, then per block bn1, bn2, block end),
    imposed instead of float64's own -- a pre-activation within rounding of zero is decided differently by any two paths, and with
    batch statistics one such element moves the gradient of its whole channel.  flips (list): receives, per ReLU, the imposed
    decisions that differ from float64's own, as (count, largest |pre-activation| among them / the map's largest |pre-activation|)."""
    it = iter(masks) if masks is not None else None

    def relu(t):
        if it is None:
            return F.relu(t)
        m = next(it).to(t.device)
        if flips is not None:
            d = m != (t.detach() > 0)
            flips.append((int(d.sum()), (t.detach().abs()[d].max() / t.detach().abs().max()).item() if d.any() else 0.0))
        return t * m

    def bn(t, name):
        if training:
            sd[name + ".num_batches_tracked"] += 1
        return F.batch_norm(t, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], training,
                            BN_MOMENTUM, CO.BN_EPS)

    p0 = "classifier_backbone."
    x = F.conv2d(x, sd[p0 + "conv1.weight"], None, stride=2, padding=3)
    x = relu(bn(x, p0 + "bn1"))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for li, (planes, blocks, stride) in enumerate(CO.LAYERS):
        for bi in range(blocks):
            p = f"{p0}layer{li + 1}.{bi}."
            s = stride if bi == 0 else 1
            idt = x
            out = relu(bn(F.conv2d(x, sd[p + "conv1.weight"]), p + "bn1"))
            out = relu(bn(F.conv2d(out, sd[p + "conv2.weight"], None, stride=s, padding=1), p + "bn2"))
            out = bn(F.conv2d(out, sd[p + "conv3.weight"]), p + "bn3")
            if bi == 0:
                idt = bn(F.conv2d(x, sd[p + "downsample.0.weight"], None, stride=s), p + "downsample.1")
            x = relu(out + idt)
    x = F.adaptive_avg_pool2d(x, (1, 1)).flatten(1)
    x = F.linear(x, sd[p0 + "fc.weight"], sd[p0 + "fc.bias"])
    return F.linear(x, sd["binary_classification_head.weight"], sd["binary_classification_head.bias"])


class OracleTrainer:
    """float64 CPU copy of the reference loop: Adam + MultiStepLR over the 163 parameters of a classifier state dict"""

    def __init__(self, sd, lr, milestones=(), gamma=1.0, betas=(0.9, 0.999), eps=1e-8):
        self.sd = OrderedDict((k, v.detach().clone().double() if v.is_floating_point() else v.detach().clone()) for k, v in sd.items())
        self.params = [self.sd[n].requires_grad_(True) for n in param_names()]
        self.opt = torch.optim.Adam(self.params, lr=lr, betas=betas, eps=eps)
        self.sched = torch.optim.lr_scheduler.MultiStepLR(self.opt, milestones=list(milestones), gamma=gamma)

    def step(self, images, labels, masks=None, flips=None):
        """-> (loss, {name: gradient}) of this step (float64); masks / flips: see forward_train"""
        self.opt.zero_grad()
        pred = torch.sigmoid(forward_train(self.sd, images.double(), masks, flips))
        loss = F.binary_cross_entropy(pred, labels.double().reshape(-1, 1))
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in zip(param_names(), self.params)}
        self.opt.step()
        self.sched.step()
        return loss.item(), grads

    def state_dict(self):
        return OrderedDict((k, v.detach().clone()) for k, v in self.sd.items())


def adam_first_step(w0, g, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's first update (step 1) of w0 by g, float64"""
    w0, g = w0.double(), g.double()
    m = (1 - betas[0]) * g
    v = (1 - betas[1]) * g * g
    return w0 - lr * (m / (1 - betas[0])) / ((v / (1 - betas[1])).sqrt() + eps)
