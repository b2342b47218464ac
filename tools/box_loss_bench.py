"""The box branch of the cascade ROI heads on the device (unmore_amd.box_loss: match_and_label -> fast_rcnn_losses with the drop-loss
weights -> next_stage_proposals, three stages) beside the NumPy / torch CPU restatement the tests compare it against
(tests/box_loss_common.py): one JSON line per run, appended to profiles/box_loss_bench.jsonl.

    python tools/box_loss_bench.py --images 16 --iters 20 --warmup 5

The input is a seeded batch of `--images` 800x1216 frames with 20 ground truths and 512 proposals each (the recipe's sampler size):
jittered ground truths, copies of them and uniform boxes; the stages use Detectron2's defaults, IoU 0.5 / 0.6 / 0.7 and weights
(10,10,5,5) / (20,20,10,10) / (30,30,15,15), drop-loss at 0.01, soft targets.  Each stage's predictions are seeded noise sized to the
proposals that reach it; the step reads the kept counts once per stage (split_proposals), as the ROI pooler of a real step would.
  step_ms / stage_ms:  a host clock around the whole step (three stages, with the backward of the six losses) and a third of it, median
                       of `--iters`, everything already on the device.
  calls_ms:            device events around each of the three calls (table upload and launches), summed over the stages, per step.
  kernels_ms:          device events around the launches alone, after the table is up: match (one launch), loss_main and loss_finish,
                       decode (decode + compaction, two launches), summed over the stages, per step.
  host_ms:             the same step through the restatement on `--threads` host threads (NumPy float32 matching, decode and drop
                       weights, torch float32 autograd for the losses)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, G, PER_IMAGE, DROP = 800, 1216, 20, 512, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_loss_bench.jsonl"))
    args = ap.parse_args()
    args.threads = min(args.threads, 16)
    from unmore_amd import box_loss as B
    from box_loss_common import (STAGE_IOUS, STAGE_WEIGHTS, droploss_iou_max_np, droploss_weights_np, losses_reference, match_np, next_stage_np,
                                 ragged_batch)
    assert torch.cuda.is_available(), "box_loss_bench needs the MI355X"
    N = args.images
    sizes = [(H, W)] * N
    images = ragged_batch(args.seed, [PER_IMAGE] * N, [G] * N, sizes, box_scale=0.3)
    rng = np.random.RandomState(args.seed + 1)
    R0 = N * PER_IMAGE
    scores = [(rng.standard_normal((R0, 2)) * 2).astype(np.float32) for _ in range(3)]
    deltas = [(rng.standard_normal((R0, 4)) * np.array(STAGE_WEIGHTS[k]) * 0.05).astype(np.float32) for k in range(3)]
    single = [int(k % 4 == 0) for k in range(N)]
    dev = torch.device("cuda:0")
    targets = [{k: torch.from_numpy(im[k]).to(dev) for k in ("gt_boxes", "gt_classes", "gt_scores")} for im in images]
    first = [torch.from_numpy(im["proposal_boxes"]).to(dev) for im in images]
    d_scores, d_deltas = [torch.from_numpy(s).to(dev) for s in scores], [torch.from_numpy(d).to(dev) for d in deltas]
    d_single = torch.tensor(single, device=dev)

    def step(timing=None, phases=None):
        props, total, rows = first, None, []
        ev = []
        for k in range(3):
            mark = (lambda: ev.append(torch.cuda.Event(enable_timing=True)) or ev[-1].record()) if timing is not None else (lambda: None)
            mark()
            matched = B.match_and_label(props, targets, STAGE_IOUS[k], 1, _phase_ms=phases)
            mark()
            R = sum(int(p.shape[0]) for p in props)
            rows.append(R)
            s, d = d_scores[k][:R].detach().requires_grad_(True), d_deltas[k][:R].detach().requires_grad_(True)
            out = B.fast_rcnn_losses(s, d, matched, box2box_weights=STAGE_WEIGHTS[k], droploss=(DROP, d_single), _phase_ms=phases)
            mark()
            loss = out["loss_cls"] + out["loss_box_reg"]
            total = loss if total is None else total + loss
            boxes, keep, counts = B.next_stage_proposals(d, matched, STAGE_WEIGHTS[k], sizes, _phase_ms=phases)
            mark()
            if k < 2:
                props = B.split_proposals(boxes, counts)
        total.backward()
        if timing is not None:
            torch.cuda.synchronize()
            for k in range(3):
                for name, i in (("match", 0), ("loss", 1), ("decode", 2)):
                    timing[name] = timing.get(name, 0.0) + ev[4 * k + i].elapsed_time(ev[4 * k + i + 1])
        return float(total.detach()), rows

    times, calls, phases = [], {}, {}
    for i in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        total, rows = step()
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    for _ in range(args.iters):
        step(timing=calls)
    for _ in range(args.iters):
        step(phases=phases)

    # ---- the restatement on the host
    torch.set_num_threads(args.threads)
    t0 = time.perf_counter()
    boxes, host_total = [im["proposal_boxes"] for im in images], 0.0
    for k in range(3):
        ms = [match_np(b, im["gt_boxes"], im["gt_classes"], im["gt_scores"], STAGE_IOUS[k]) for b, im in zip(boxes, images)]
        R = sum(len(b) for b in boxes)
        gtb = [m["gt_boxes"] for m in ms]
        w = droploss_weights_np(droploss_iou_max_np(deltas[k][:R], boxes, gtb, STAGE_WEIGHTS[k]), DROP, single, N)
        lc, lb, _, _, _ = losses_reference(scores[k][:R], deltas[k][:R], np.concatenate(boxes), np.concatenate(gtb),
                                           np.concatenate([m["gt_classes"] for m in ms]), np.concatenate([m["gt_scores"] for m in ms]), w,
                                           STAGE_WEIGHTS[k], dtype=torch.float32)
        host_total += lc + lb
        clipped, keep, counts = next_stage_np(deltas[k][:R], boxes, STAGE_WEIGHTS[k], sizes)
        at, nxt = 0, []
        for c in clipped:
            nxt.append(c[keep[at:at + len(c)]])
            at += len(c)
        boxes = nxt
    host_ms = (time.perf_counter() - t0) * 1e3
    step_ms = statistics.median(times)
    line = {"tool": "box_loss_bench", "images": N, "hw": [H, W], "gts_per_image": G, "proposals_per_image": PER_IMAGE, "rows_per_stage": rows,
            "iters": args.iters, "warmup": args.warmup, "step_ms": round(step_ms, 3), "stage_ms": round(step_ms / 3, 3),
            "calls_ms": {k: round(v / args.iters, 4) for k, v in calls.items()},
            "kernels_ms": {k: round(v / args.iters, 4) for k, v in phases.items()},
            "losses_sum": total, "losses_sum_host_float32": host_total, "host_threads": args.threads, "host_ms": round(host_ms, 1),
            "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
