"""Existence-classifier training items (synthesize_classifier_items) against the step that consumes them: one JSON line per run,
appended to profiles/clf_items_bench.jsonl.

    python tools/clf_items_bench.py --batch 20  --size 128 --iters 20 --warmup 3
    python tools/clf_items_bench.py --batch 256 --size 128 --iters 10 --warmup 2

items_per_s: device-synchronised wall time of `iters` calls on `batch` synthetic 500x375 sources already on the GPU (random
image, ellipse masks), coins and crop boxes drawn as in training (Python's `random`, torch's CPU generator) -- the whole call:
table upload, background pass, the one read-back, crop + resize.
cpu_items_per_s: the CPU restatement of the same item (tests/clf_items_common.py: numpy row scans standing in for
cv2.distanceTransform, F.interpolate for torchvision's resize) in `--cpu-workers` single-threaded worker processes, as a
DataLoader runs them.  It is NOT cv2's speed: OpenCV's C loop is faster than numpy row scans, so this line bounds the host path
from below only loosely; it is here because cv2 is not installed where this tool was written.
step_images_per_s: ClassifierTrainStep (bf16 unless --dtype fp32) on the same batch and size, for comparison.
The CPU leg runs first, in spawned processes that never open the GPU."""
import argparse
import json
import multiprocessing as mp
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 375, 500


def make_item(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]

    def ell():
        cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
        ry, rx = rng.uniform(H / 10, H / 3), rng.uniform(W / 10, W / 3)
        return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1)

    top1 = ell()
    full = top1 | ell()
    return (torch.from_numpy(rng.random((3, H, W)).astype(np.float32)), torch.from_numpy(top1.astype(np.uint8) * 255),
            torch.from_numpy(full.astype(np.uint8) * 255))


def _cpu_worker(args):
    seed, S = args
    torch.set_num_threads(1)
    import clf_items_common as C
    from unmore_amd.labels import random_resized_crop_params
    img, top1, full = make_item(seed)
    random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    t0 = time.perf_counter()
    coin = random.random() < 0.5
    C.classifier_item(img, top1, full, coin, random_resized_crop_params(H, W, ratio=(3 / 4, 4 / 3), generator=g), S)
    return time.perf_counter() - t0


def cpu_leg(n_items, S, workers):
    ctx = mp.get_context("spawn")
    with ctx.Pool(workers) as pool:
        pool.map(_cpu_worker, [(10_000 + k, S) for k in range(workers)])          # warm-up: imports
        t0 = time.perf_counter()
        per = pool.map(_cpu_worker, [(k, S) for k in range(n_items)], chunksize=1)
        wall = time.perf_counter() - t0
    return {"cpu_items": n_items, "cpu_workers": workers, "cpu_items_per_s": round(n_items / wall, 1),
            "cpu_ms_per_item_one_worker": round(1e3 * sum(per) / len(per), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="bf16")
    ap.add_argument("--cpu-items", type=int, default=512, help="0 = skip the CPU leg")
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clf_items_bench.jsonl"))
    a = ap.parse_args()
    B, S = a.batch, a.size
    rec = {"tool": "clf_items_bench", "batch": B, "size": S, "source_hw": [H, W], "iters": a.iters, "warmup": a.warmup}
    if a.cpu_items > 0:
        rec.update(cpu_leg(a.cpu_items, S, a.cpu_workers))

    from unmore_amd import ClassifierTrainStep, synthesize_classifier_items
    dev = torch.device("cuda:0")
    base = [make_item(k) for k in range(min(B, 32))]
    items = [tuple(t.to(dev) for t in base[k % len(base)]) for k in range(B)]
    imgs, top1, full = ([it[j] for it in items] for j in range(3))
    random.seed(0)
    g = torch.Generator().manual_seed(0)
    for _ in range(a.warmup):
        out, labels, info = synthesize_classifier_items(imgs, top1, full, S, generator=g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_bg = 0
    for _ in range(a.iters):
        out, labels, info = synthesize_classifier_items(imgs, top1, full, S, generator=g)
        n_bg += B - int(info["branch"].sum().item())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.iters * 1e3
    rec.update({"ms_per_batch": round(ms, 3), "items_per_s": round(B / ms * 1e3, 1), "background_fraction": round(n_bg / (B * a.iters), 3),
                "positive_fraction": round(float(labels.mean().item()), 3)})
    if not a.no_step:
        from oracle import classifier_oracle as CO
        from unmore_amd.binary_classifier import Binary_Classifier
        from unmore_amd.hashrng import uniform
        dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
        net = Binary_Classifier(device="cuda:0", image_size=S, args=None, compute_dtype=dt)
        net.load_state_dict(CO.hash_state("clf", uniform), strict=True)
        net = net.to(dev).train()
        step = ClassifierTrainStep(net, lr=1e-4)
        for _ in range(max(a.warmup, 3)):
            step.step(out, labels)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            loss = step.step(out, labels)
        torch.cuda.synchronize()
        sms = (time.perf_counter() - t0) / a.iters * 1e3
        rec.update({"step_dtype": a.dtype, "step_ms": round(sms, 3), "step_images_per_s": round(B / sms * 1e3, 1),
                    "items_over_step": round(sms / ms, 2), "loss": float(loss.item())})
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
