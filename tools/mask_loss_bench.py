"""Mask-head targets and the score-weighted mask loss on the device (unmore_amd.mask_loss.mask_rcnn_loss_weighted) beside the NumPy /
torch CPU restatement the tests compare it against (tests/mask_loss_common.py): one JSON line per run, appended to
profiles/mask_loss_bench.jsonl.

    python tools/mask_loss_bench.py --images 16 --iters 10 --warmup 3

The input is a seeded batch of `--images` 800x1216 frames with 20 elliptic blob masks each and 128 proposals per image (512 ROIs x
0.25 foreground, the recipe's sampler), which are ground-truth boxes moved by up to 15 % of their size; side 28, one channel, weights
uniform in [0.2, 1].
  device_ms:    per logit type, the whole call with everything already on the device -- host checks and the table, one upload, the
                launches -- plus the backward that scales the saved gradient, as a host clock around it, median of `--iters`.
  kernels_ms:   device events around the two parts: targets_loss (targets, loss terms, gradient, one partial per proposal) and finish.
  alone_ms:     targets_loss for ONE proposal on its own, the batch's largest box and a box the size of the frame: the longest a launch
                can wait for its last proposal (a proposal's samples grow with its area; above 65536 samples four workgroups share it).
  host_ms:      mask_targets_np (float32) on `--threads` host threads, then loss_reference (float64 torch, the same thread count).
                The step stops taking new proposals after `--host-seconds`; `host_proposals` says how many it did.
`targets_differing` counts the bins on which the device and the float32 restatement disagree."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, G, PER_IMAGE, SIDE = 800, 1216, 20, 128, 28


def make_image(rng):
    from mask_loss_common import jittered_proposals
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    masks = np.zeros((G, H, W), dtype=bool)
    for k in range(G):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, 200), rng.uniform(20, 300)
        masks[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    boxes, idx = jittered_proposals(rng, masks, PER_IMAGE)
    return {"gt_masks": masks, "proposal_boxes": boxes, "mask_index": idx}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-seconds", type=float, default=150.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_loss_bench.jsonl"))
    args = ap.parse_args()
    args.threads = min(args.threads, 16)
    from unmore_amd.mask_loss import mask_rcnn_loss_weighted
    from mask_loss_common import loss_reference, mask_targets_np
    assert torch.cuda.is_available(), "mask_loss_bench needs the MI355X"

    rng = np.random.RandomState(args.seed)
    images = [make_image(rng) for _ in range(args.images)]
    R = args.images * PER_IMAGE
    logits = (rng.standard_normal((R, 1, SIDE, SIDE)) * 3).astype(np.float32)
    weights = rng.uniform(0.2, 1.0, size=R).astype(np.float32)
    dev = [{k: torch.from_numpy(v).cuda() for k, v in im.items()} for im in images]
    w = torch.from_numpy(weights).cuda()
    areas = np.concatenate([(im["proposal_boxes"][:, 2] - im["proposal_boxes"][:, 0]) * (im["proposal_boxes"][:, 3] - im["proposal_boxes"][:, 1])
                            for im in images])

    device_ms, kernels_ms, losses, targets = {}, {}, {}, None
    for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        x = torch.from_numpy(logits).cuda().to(dtype).requires_grad_(True)
        times, phases = [], {}
        for i in range(args.warmup + args.iters):
            x.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = {}
            loss = mask_rcnn_loss_weighted(x, dev, w, stats=stats)
            loss.backward()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
                mask_rcnn_loss_weighted(x, dev, w, _phase_ms=phases)
        device_ms[name] = round(statistics.median(times), 3)
        kernels_ms[name] = {k: round(v / args.iters, 4) for k, v in phases.items()}
        losses[name] = loss.item()
        if targets is None:
            targets, counters = stats["targets"].cpu().numpy(), stats["counters"].cpu().numpy().tolist()

    # ---- one proposal on its own
    big = int(np.argmax(areas))
    alone_ms = {}
    for name, k, box, idx in (("largest_box", big // PER_IMAGE, images[big // PER_IMAGE]["proposal_boxes"][big % PER_IMAGE],
                               images[big // PER_IMAGE]["mask_index"][big % PER_IMAGE]),
                              ("frame_sized_box", 0, np.array([0, 0, W, H], dtype=np.float32), np.int64(0))):
        inst = [{"gt_masks": dev[k]["gt_masks"], "proposal_boxes": torch.from_numpy(np.asarray(box)[None]).cuda(),
                 "mask_index": torch.from_numpy(np.asarray(idx)[None]).cuda()}]
        x1, phases = torch.from_numpy(logits[:1]).cuda(), {}
        for i in range(args.warmup + args.iters):
            mask_rcnn_loss_weighted(x1, inst, w[:1], _phase_ms=phases if i >= args.warmup else None)
        alone_ms[name] = round(phases["targets_loss"] / args.iters, 4)

    # ---- the restatement on the host, proposals spread over the threads
    torch.set_num_threads(args.threads)
    jobs = [(k, r) for k in range(args.images) for r in range(PER_IMAGE)]
    deadline = time.perf_counter() + args.host_seconds

    def one(job):
        k, r = job
        if time.perf_counter() > deadline:
            return None
        im = images[k]
        return mask_targets_np(im["gt_masks"], im["proposal_boxes"][r:r + 1], im["mask_index"][r:r + 1], SIDE, np.float32)[0]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(args.threads) as pool:
        host_targets = list(pool.map(one, jobs))
    done = [i for i, t in enumerate(host_targets) if t is not None]
    t_host = np.stack([host_targets[i] for i in done])
    loss_reference(logits[done], t_host, None, weights[done])
    host_ms = (time.perf_counter() - t0) * 1e3
    loss64, _, _ = loss_reference(logits, targets, None, weights)
    line = {"tool": "mask_loss_bench", "images": args.images, "hw": [H, W], "masks_per_image": G, "proposals": R, "side": SIDE,
            "iters": args.iters, "warmup": args.warmup, "median_box_area": float(np.median(areas)), "max_box_area": float(areas.max()),
            "device_ms": device_ms, "kernels_ms": kernels_ms, "alone_ms": alone_ms, "loss": losses, "loss_float64_on_device_targets": loss64, "counters": counters,
            "host_threads": args.threads, "host_ms": round(host_ms, 1), "host_proposals": len(done),
            "targets_differing": int((targets[done] != t_host).sum()), "bins_compared": int(t_host.size),
            "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
