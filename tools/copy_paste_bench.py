"""Copy-paste augmentation of a detector batch on the device (unmore_amd.copy_paste.copy_and_paste) beside the torch CPU restatement the
tests compare it against (tests/copy_paste_common.py::copy_paste_reference, the reference's own ops): one JSON line per run, appended to
profiles/copy_paste_bench.jsonl.

    python tools/copy_paste_bench.py --pairs 16 --iters 10 --warmup 3

The input is a seeded batch of `--pairs` 800x1216 frames with 20 elliptic blob masks each, paired with its own reverse as the reference's
run_step pairs it, with the stage-3 recipe's draws (rate 1.0, random count, ratio 0.3-1.0) made once.
  device_ms:         the whole call with the batch already on the device -- host checks and tables, one upload, the launches, the
                     read-back, the output views -- as a host clock around it, median of `--iters`.
  device_upload_ms:  the same including the host-to-device copy of the batch's images, masks and boxes.
  kernels_ms:        device events around the three parts: resize_paste (bit sets of the pasted and the existing masks), overlap
                     (intersections, areas, keep decision), compose (alpha, image, output masks, areas and boxes).
  host_ms:           copy_paste_reference on `--threads` host threads.
`equal_to_restatement`: masks, boxes and sources equal, image bytes within one level."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, N = 800, 1216, 20


def make_item(rng):
    img = torch.from_numpy(rng.randint(0, 256, (3, H, W)).astype(np.uint8))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    masks = np.zeros((N, H, W), dtype=bool)
    boxes = np.zeros((N, 4), dtype=np.float32)
    for k in range(N):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, 200), rng.uniform(20, 300)
        masks[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        ys, xs = np.nonzero(masks[k])
        boxes[k] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if ys.size else 0
    return {"image": img, "masks": torch.from_numpy(masks), "boxes": torch.from_numpy(boxes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_paste_bench.jsonl"))
    args = ap.parse_args()
    from unmore_amd.copy_paste import copy_and_paste, draw_params
    from copy_paste_common import copy_paste_reference
    assert torch.cuda.is_available(), "copy_paste_bench needs the MI355X"

    rng = np.random.RandomState(args.seed)
    items = [make_item(rng) for _ in range(args.pairs)]
    params = draw_params([N] * args.pairs, [(H, W)] * args.pairs, 1.0, True, 0.3, 1.0, py_random=random.Random(args.seed),
                         np_random=np.random.RandomState(args.seed))
    pinned = [{k: v.pin_memory() for k, v in it.items()} for it in items]

    def upload():
        return [{k: v.to("cuda", non_blocking=True) for k, v in it.items()} for it in pinned]

    dev = upload()
    torch.cuda.synchronize()
    t_dev, t_up, phases = [], [], {}
    for i in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = copy_and_paste(dev[::-1], dev, params)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d2 = upload()
        out2 = copy_and_paste(d2[::-1], d2, params)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del out2, d2
        if i >= args.warmup:
            t_dev.append((t1 - t0) * 1e3)
            t_up.append((t2 - t1) * 1e3)
            copy_and_paste(dev[::-1], dev, params, _phase_ms=phases)
    kernels = {k: round(v / args.iters, 4) for k, v in phases.items()}

    torch.set_num_threads(args.threads)
    copy_paste_reference(items[::-1][:1], items[:1], params[:1])
    t0 = time.perf_counter()
    ref = copy_paste_reference(items[::-1], items, params)
    host_ms = (time.perf_counter() - t0) * 1e3
    equal = True
    for g, r in zip(out, ref):
        equal &= (g["image"] is not None) and torch.equal(g["masks"].cpu().bool(), r["masks"].bool()) and torch.equal(g["boxes"].cpu(), r["boxes"])
        equal &= torch.equal(g["source"].cpu(), r["source"]) and int((g["image"].cpu().int() - r["image"].int()).abs().max()) <= 1
    line = {"tool": "copy_paste_bench", "pairs": args.pairs, "hw": [H, W], "masks_per_image": N, "iters": args.iters, "warmup": args.warmup,
            "copies": [0 if p is None else int(p[0].size) for p in params], "instances_out": [int(g["masks"].shape[0]) for g in out],
            "device_ms": round(statistics.median(t_dev), 3), "device_upload_ms": round(statistics.median(t_up), 3), "kernels_ms": kernels,
            "host_threads": args.threads, "host_ms": round(host_ms, 1), "equal_to_restatement": bool(equal),
            "device_over_host": round(host_ms / statistics.median(t_dev), 1), "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
