"""Existence-classifier training step (ClassifierTrainStep) throughput: one JSON line per run.

    python tools/clf_train_bench.py --batch 20 --size 128 --dtype bf16 --steps 20 --warmup 5 --graphs on [--cpu-baseline]

ms per step is device-synchronised wall time over `steps` steps after `warmup` (graph capture, when on, happens in the warm-up).
GFLOP per image is counted from the layer shapes: 2 * MAC of every convolution and Linear layer, three times (forward, data
gradient, weight gradient) except the stem's data gradient, which the step does not compute.  The fp32 mode's GEMMs run as three
bf16 products (umr_set_f32_mode 'x3'), so its dense peak is the bf16 peak / 6 (six plane pairs per product, bench.py's convention).
--cpu-baseline: the float32 PyTorch step (autograd, nn.BatchNorm2d training mode, BCELoss, Adam) of the same model on the host's
16 threads, median of 5 after 2 warm-ups."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0    # dense bf16 MFMA (MI355X spec)
LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))


def _down2(n):
    return (n - 1) // 2 + 1


def flops_per_image(H, W):
    """(training-step FLOP, forward MAC) per image of ResNet-50 + Linear(1000, 1) at H x W"""
    macs = []
    H1, W1 = _down2(H), _down2(W)
    stem = H1 * W1 * 64 * 3 * 49
    h, w = _down2(H1), _down2(W1)
    cin = 64
    for planes, blocks, stride in LAYERS:
        for bi in range(blocks):
            s = stride if bi == 0 else 1
            ho, wo = (_down2(h), _down2(w)) if s == 2 else (h, w)
            macs += [h * w * cin * planes, ho * wo * planes * planes * 9, ho * wo * planes * planes * 4]
            if bi == 0:
                macs.append(ho * wo * cin * planes * 4)
            h, w, cin = ho, wo, planes * 4
    macs += [2048 * 1000, 1000]
    fwd = stem + sum(macs)
    return 2 * (3 * fwd - stem), fwd


def _cpu_forward(net, x):
    rb = net.classifier_backbone
    x = F.max_pool2d(F.relu(rb.bn1(rb.conv1(x))), 3, 2, 1)
    for li in range(4):
        for blk in getattr(rb, f"layer{li + 1}"):
            out = F.relu(blk.bn1(blk.conv1(x)))
            out = F.relu(blk.bn2(blk.conv2(out)))
            out = blk.bn3(blk.conv3(out))
            idt = blk.downsample[1](blk.downsample[0](x)) if blk.downsample is not None else x
            x = F.relu(out + idt)
    x = rb.fc(F.adaptive_avg_pool2d(x, 1).flatten(1))
    return torch.sigmoid(net.binary_classification_head(x))


def cpu_baseline(B, S, threads=16):
    from oracle import classifier_oracle as CO
    from unmore_amd.binary_classifier import Binary_Classifier
    from unmore_amd.hashrng import uniform
    torch.set_num_threads(threads)
    net = Binary_Classifier(device="cpu", image_size=S, args=None)
    net.load_state_dict(CO.hash_state("clf", uniform), strict=True)
    # the stride-2 3x3 convs of the holder modules are torchvision's (stride on conv2, padding 1)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    x = torch.rand(B, 3, S, S)
    y = (torch.arange(B) % 2).float().view(B, 1)
    times = []
    for i in range(7):
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = F.binary_cross_entropy(_cpu_forward(net, x), y)
        loss.backward()
        opt.step()
        times.append(time.perf_counter() - t0)
    ms = statistics.median(times[2:]) * 1e3
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        model = platform.processor()
    return {"cpu_ms_per_step": round(ms, 2), "cpu_images_per_s": round(B / ms * 1e3, 2), "cpu_threads": torch.get_num_threads(),
            "cpu_model": model}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="bf16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", choices=("on", "off", "auto"), default="auto")
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    from oracle import classifier_oracle as CO
    from unmore_amd import ClassifierTrainStep
    from unmore_amd.binary_classifier import Binary_Classifier
    from unmore_amd.hashrng import uniform
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    net = Binary_Classifier(device="cuda:0", image_size=a.size, args=None, compute_dtype=dt)
    net.load_state_dict(CO.hash_state("clf", uniform), strict=True)
    net = net.to(dev).train()
    step = ClassifierTrainStep(net, lr=1e-4).set_graph_mode(a.graphs)
    B, S = a.batch, a.size
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    y = (torch.arange(B) % 2).float().view(B, 1).to(dev)
    for _ in range(a.warmup):
        step.step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step.step(x, y)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    fl, fwd_mac = flops_per_image(S, S)
    tflops = fl * B / (ms * 1e-3) / 1e12
    peak = PEAK_BF16_TFLOPS if a.dtype == "bf16" else PEAK_BF16_TFLOPS / 6.0
    rec = {"tool": "clf_train_bench", "batch": B, "size": S, "dtype": a.dtype, "graphs": a.graphs, "steps": a.steps, "warmup": a.warmup,
           "graph_replays": step.graph_replays, "ms_per_step": round(ms, 3), "images_per_s": round(B / ms * 1e3, 1),
           "gflop_per_image": round(fl / 1e9, 3), "fwd_gmac_per_image": round(fwd_mac / 1e9, 3), "tflops": round(tflops, 2),
           "peak_tflops": peak, "fraction_of_peak": round(tflops / peak, 4), "loss": float(loss.item()),
           "device": torch.cuda.get_device_name(0)}
    if a.cpu_baseline:
        rec.update(cpu_baseline(B, S))
        rec["speedup_vs_cpu"] = round(rec["cpu_ms_per_step"] / ms, 1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
