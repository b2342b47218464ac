"""The ROI heads' proposal sampling on the device (unmore_amd.roi_sample.label_and_sample_proposals) beside the torch-ops composition of
the same steps and the NumPy restatement: one JSON line, appended to profiles/roi_sample_bench.jsonl.

    python tools/roi_sample_bench.py --images 16 --windows 5 --iters 400 --warmup 20

The workload is the recipe's: `--images` frames of 800x1216, 2 000 seeded proposals (a third of them jittered ground truths) and 20
ground truths per image, appended; threshold 0.5, B = 512 at fraction 0.25.  Every time is the median over `--windows` windows of the
mean over `--iters` calls, a host clock around work that ends in a device synchronise:
  list_call_ms:     label_and_sample_proposals in its list form (checks, the table upload, two launches, the read of the counts).
  padded_call_ms:   the padded form, which reads nothing back.
  launch_ms:        device events around each launch alone (match, select), the mean over `--iters` calls.
  torch_ms:         the torch ops of Detectron2's label_and_sample_proposals on the GPU: per image the cat with the ground truths, the
                    [G, R] IoU matrix, max, two nonzero and two randperm, the gathers of every field, and the two .item() reads.
  numpy_ms:         the NumPy restatement (tests/roi_sample_common.py), images spread over `--procs` processes, one run."""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

H, W, R, G, B, FRACTION, THRESHOLD = 800, 1216, 2000, 20, 512, 0.25, 0.5


def _batch(N, seed):
    rng = np.random.RandomState(seed)
    props, tgts = [], []
    for _ in range(N):
        side = np.exp(rng.uniform(np.log(24.0), np.log(0.8 * H), G))
        aspect = np.exp(rng.uniform(np.log(0.5), np.log(2.0), G))
        bw, bh = np.minimum(side / np.sqrt(aspect), W), np.minimum(side * np.sqrt(aspect), H)
        x1, y1 = rng.uniform(0, 1, G) * (W - bw), rng.uniform(0, 1, G) * (H - bh)
        gt = np.stack([x1, y1, x1 + bw, y1 + bh], axis=1).astype(np.float32)
        pw, ph = rng.uniform(16, 400, R), rng.uniform(16, 400, R)
        px, py = rng.uniform(0, 1, R) * (W - pw), rng.uniform(0, 1, R) * (H - ph)
        p = np.stack([px, py, px + pw, py + ph], axis=1).astype(np.float32)
        for j in range(0, R, 3):
            g = gt[rng.randint(G)]
            p[j] = g + rng.uniform(-0.15, 0.15, 4).astype(np.float32) * np.array([g[2] - g[0], g[3] - g[1]] * 2, np.float32)
        props.append((p, rng.standard_normal(R).astype(np.float32)))
        tgts.append({"gt_boxes": gt, "gt_classes": np.zeros(G, np.int64), "gt_scores": rng.uniform(0.1, 1.0, G).astype(np.float32)})
    return props, tgts


def _numpy_image(args):
    import roi_sample_common as C
    prop, tgt, seed = args
    r = C.label_and_sample_np([prop], [tgt], THRESHOLD, 1, B, FRACTION, seed=seed)[0]
    # the hash takes the image's index: image n of the batch is image 0 here, so only the counts are compared with the device
    return r["counters"].tolist()


def _windows_ms(fn, windows, iters, warmup, sync):
    """the median over the windows of the mean call time, and the last result"""
    out = None
    for _ in range(warmup):
        out = fn()
    means = []
    for _ in range(windows):
        sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = fn()
        sync()
        means.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(means), out


def _torch_step(props, tgts, gt_logit):
    """Detectron2's label_and_sample_proposals in torch ops"""
    import torch
    out, n_fg, n_bg = [], [], []
    for (boxes, logits), t in zip(props, tgts):
        gt = t["gt_boxes"]
        boxes, logits = torch.cat([boxes, gt]), torch.cat([logits, gt_logit * torch.ones(len(gt), device=gt.device)])
        g_area, b_area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        wh = (torch.min(gt[:, None, 2:], boxes[:, 2:]) - torch.max(gt[:, None, :2], boxes[:, :2])).clamp_(min=0)
        inter = wh.prod(dim=2)
        m = torch.where(inter > 0, inter / (g_area[:, None] + b_area - inter), torch.zeros(1, dtype=inter.dtype, device=inter.device))
        vals, idx = m.max(dim=0)
        classes = t["gt_classes"][idx]
        classes[vals < THRESHOLD] = 1
        positive, negative = ((classes != -1) & (classes != 1)).nonzero().squeeze(1), (classes == 1).nonzero().squeeze(1)
        num_pos = min(positive.numel(), int(B * FRACTION))
        num_neg = min(negative.numel(), B - num_pos)
        sampled = torch.cat([positive[torch.randperm(positive.numel(), device=gt.device)[:num_pos]],
                             negative[torch.randperm(negative.numel(), device=gt.device)[:num_neg]]])
        target = idx[sampled]
        item = {"proposal_boxes": boxes[sampled], "objectness_logits": logits[sampled], "gt_classes": classes[sampled],
                "gt_boxes": gt[target], "gt_scores": t["gt_scores"][target]}
        n_bg.append((item["gt_classes"] == 1).sum().item())
        n_fg.append(item["gt_classes"].numel() - n_bg[-1])
        out.append(item)
    return out, (sum(n_fg) / len(n_fg), sum(n_bg) / len(n_bg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_sample_bench.jsonl"))
    args = ap.parse_args()
    args.procs = max(1, min(args.procs, 16))
    pool = None
    if not args.skip_numpy:
        pool = multiprocessing.get_context("spawn").Pool(args.procs)          # fresh processes that never open the GPU, before this one does
        pool.map(abs, range(args.procs))
    import torch
    from unmore_amd import roi_sample
    assert torch.cuda.is_available(), "roi_sample_bench needs the MI355X"
    dev = torch.device("cuda:0")
    N = args.images
    sync = torch.cuda.synchronize
    props_np, tgts_np = _batch(N, args.seed)
    props = [(torch.from_numpy(b).to(dev), torch.from_numpy(l).to(dev)) for b, l in props_np]
    tgts = [{k: torch.from_numpy(v).to(dev) for k, v in t.items()} for t in tgts_np]
    call = lambda **kw: roi_sample.label_and_sample_proposals(props, tgts, iou_threshold=THRESHOLD, batch_size_per_image=B,     # noqa: E731
                                                              positive_fraction=FRACTION, seed=args.seed, **kw)
    list_ms, samples = _windows_ms(call, args.windows, args.iters, args.warmup, sync)
    padded_ms, _ = _windows_ms(lambda: call(padded=True), args.windows, args.iters, args.warmup, sync)
    phases, st = {}, {}
    calls = args.iters
    for _ in range(calls):
        call(padded=True, stats=st, _phase_ms=phases)
    counters = st["counters"].cpu().numpy()
    torch_ms, tout = _windows_ms(lambda: _torch_step(props, tgts, roi_sample.GT_LOGIT), args.windows, args.iters, args.warmup, sync)
    numpy_ms = None
    if pool is not None:
        t0 = time.perf_counter()
        res = pool.map(_numpy_image, [(props_np[n], tgts_np[n], args.seed) for n in range(N)])
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same = [r[:2] + r[4:] == counters[n, [0, 1, 4]].tolist() and r[2:4] == counters[n, 2:4].tolist() for n, r in enumerate(res)]
        print(f"# numpy restatement: {sum(same)} of {N} images have the device's counters", file=sys.stderr)
        pool.close()
        pool.join()
    line = {"tool": "roi_sample_bench", "images": N, "frame_hw": [H, W], "proposals_per_image": R, "gt_per_image": G,
            "batch_size_per_image": B, "positive_fraction": FRACTION, "windows": args.windows, "iters": args.iters, "warmup": args.warmup,
            "list_call_ms": round(list_ms, 4), "padded_call_ms": round(padded_ms, 4),
            "launch_ms": {k: round(v / calls, 4) for k, v in phases.items()}, "launches_ms": round(sum(phases.values()) / calls, 4),
            "torch_ms": round(torch_ms, 4), "numpy_ms": None if numpy_ms is None else round(numpy_ms, 1),
            "numpy_procs": args.procs if numpy_ms is not None else 0, "positives": int(counters[:, 0].sum()),
            "negatives": int(counters[:, 1].sum()), "sampled_fg": int(counters[:, 2].sum()), "sampled_bg": int(counters[:, 3].sum()),
            "samples": [sum(c) for c in samples.counts][:4], "torch_fg_bg": list(tout[1]), "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
