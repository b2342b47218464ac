"""The ROI pooler on the device (unmore_amd.roi_pool.ROIPooler: prepare -> forward -> backward) beside a composition of torch ops on the
same GPU and the NumPy restatement the tests compare it against (tests/roi_pool_common.py): one JSON line per run, appended to
profiles/roi_pool_bench.jsonl.

    python tools/roi_pool_bench.py --images 16 --iters 20 --warmup 5

The input is the recipe's: `--images` frames of 800 x 1216 under the levels p2..p5 (maps of 200 x 304 ... 25 x 38), 256 channels, 512
proposals per image drawn as tools/box_loss_bench.py draws them, output sides 7 (a box stage) and 14 (the mask head), float32 and
bfloat16 maps.  Per (side, type):
  forward_ms / backward_ms:  a host clock around ROIPooler.forward and around out.backward, median of `--iters`, everything on the device.
  kernels_ms:                device events around each launch alone: prepare (image and level per box), forward, backward.
  bytes:                     what each launch must move: forward = the output plus every feature element under some box's taps, once;
                             backward = the output gradient plus every feature map, written whole; floor_ms = those bytes at `--hbm-tbs`.
  torch_ops_ms:              the same pooling by torch ops at sampling ratio 2: per level the boxes are gathered with nonzero (a host
                             read, as the original's), sampled with F.grid_sample(align_corners=True) image by image and averaged with
                             avg_pool2d(2); forward and backward.  (Its border rule is grid_sample's zero padding, not roi_align's
                             clamp: a timing arm, not a comparator.)  ratio2_ms: the device module at sampling ratio 2, for like with like.
  host_ms:                   the float64 restatement, forward and adjoint, on `--procs` processes (side 7, float32 only)."""
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

FRAME, STRIDES, C, PER_IMAGE = (800, 1216), (4, 8, 16, 32), 256, 512
SCALES = tuple(1.0 / s for s in STRIDES)


def _host_image(job):
    """one image through the restatement: forward and adjoint on every level (a worker process; nothing of the GPU is touched)"""
    from roi_pool_common import pooler_adjoint_np, pooler_np
    seed, boxes, P = job
    rng = np.random.RandomState(seed)
    maps = [rng.standard_normal((1, C, FRAME[0] // s, FRAME[1] // s)).astype(np.float32) for s in STRIDES]
    t0 = time.perf_counter()
    out = pooler_np(maps, [boxes], P, SCALES)
    pooler_adjoint_np(out, [m.shape for m in maps], [boxes], P, SCALES)
    return time.perf_counter() - t0


def _touched_elements(box_lists, levels_per_image):
    """feature elements (per channel) under the taps of some box: the union of the boxes' tap rectangles per image and level"""
    total = 0
    for boxes, levels in zip(box_lists, levels_per_image):
        for l, s in enumerate(STRIDES):
            H, W = FRAME[0] // s, FRAME[1] // s
            seen = np.zeros((H, W), dtype=bool)
            for b in boxes[levels == l]:
                x0, y0 = int(np.floor(b[0] / s - 0.5)), int(np.floor(b[1] / s - 0.5))
                x1, y1 = int(np.ceil(b[2] / s - 0.5)) + 1, int(np.ceil(b[3] / s - 0.5)) + 1
                seen[max(y0, 0):max(min(y1, H), 0), max(x0, 0):max(min(x1, W), 0)] = True
            total += int(seen.sum())
    return total


def _torch_ops_pool(x, boxes, levels, P, first):
    """sampling ratio 2 by torch ops: [R,C,P,P]"""
    import torch
    import torch.nn.functional as F
    out = x[0].new_zeros((boxes.shape[0], x[0].shape[1], P, P))
    image = torch.bucketize(torch.arange(boxes.shape[0], device=boxes.device), first[1:].long(), right=True)
    steps = (torch.arange(2 * P, device=boxes.device, dtype=torch.float32) + 0.5) / (2 * P)
    for l, f in enumerate(x):
        H, W = f.shape[2:]
        for n in range(f.shape[0]):
            rows = torch.nonzero((levels == l) & (image == n))[:, 0]                     # the host read of the original
            if rows.numel() == 0:
                continue
            b = boxes[rows] * SCALES[l] - 0.5
            xs = b[:, 0:1] + (b[:, 2:3] - b[:, 0:1]) * steps[None]                          # [R, 2P]
            ys = b[:, 1:2] + (b[:, 3:4] - b[:, 1:2]) * steps[None]
            grid = torch.stack([(2 * xs / (W - 1) - 1)[:, None, :].expand(-1, 2 * P, -1), (2 * ys / (H - 1) - 1)[:, :, None].expand(-1, -1, 2 * P)], -1)
            s = F.grid_sample(f[n:n + 1], grid.reshape(1, -1, 2 * P, 2).to(f.dtype), mode="bilinear", align_corners=True)
            out[rows] = F.avg_pool2d(s, 2)[0].reshape(f.shape[1], -1, P, P).transpose(0, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM rate the floors are priced at, TB/s (MI355X: 8)")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_pool_bench.jsonl"))
    args = ap.parse_args()
    args.procs = min(args.procs, 16)
    from roi_pool_common import assign_levels, recipe_batch
    N = args.images
    box_lists = recipe_batch(args.seed, N, PER_IMAGE, FRAME)
    levels_np = [assign_levels(b, 2, 5) for b in box_lists]

    # ---- the restatement first, in fresh processes, before this one opens the GPU
    host_ms = None
    if not args.skip_host:
        t0 = time.perf_counter()
        with multiprocessing.get_context("spawn").Pool(args.procs) as pool:
            pool.map(_host_image, [(args.seed + k, b, 7) for k, b in enumerate(box_lists)])
        host_ms = (time.perf_counter() - t0) * 1e3

    import torch
    from unmore_amd import roi_pool as R
    assert torch.cuda.is_available(), "roi_pool_bench needs the MI355X"
    dev = torch.device("cuda:0")
    boxes = [torch.from_numpy(b).to(dev) for b in box_lists]
    cat = torch.cat(boxes)
    first = torch.tensor(np.cumsum([0] + [len(b) for b in box_lists]), dtype=torch.int32, device=dev)
    levels = torch.from_numpy(np.concatenate(levels_np)).to(dev)
    touched = _touched_elements(box_lists, levels_np)
    map_elements = N * C * sum((FRAME[0] // s) * (FRAME[1] // s) for s in STRIDES)
    rows = N * PER_IMAGE
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    cases = {}
    for P in (7, 14):
        for dtype in (torch.float32, torch.bfloat16):
            x = [torch.randn((N, C, FRAME[0] // s, FRAME[1] // s), device=dev, generator=gen).to(dtype).requires_grad_(True) for s in STRIDES]
            g = torch.randn((rows, C, P, P), device=dev, generator=gen).to(dtype)

            def timed(fn_fwd, iters, warmup):
                fwd, bwd = [], []
                for i in range(warmup + iters):
                    for t in x:
                        t.grad = None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn_fwd()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    out.backward(g)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if i >= warmup:
                        fwd.append((t1 - t0) * 1e3)
                        bwd.append((t2 - t1) * 1e3)
                return round(statistics.median(fwd), 4), round(statistics.median(bwd), 4)

            pooler, pooler2 = R.ROIPooler(P, SCALES, 0), R.ROIPooler(P, SCALES, 2)
            fwd_ms, bwd_ms = timed(lambda: pooler(x, boxes), args.iters, args.warmup)
            r2_fwd, r2_bwd = timed(lambda: pooler2(x, boxes), args.iters, args.warmup)
            phases = {}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(args.iters):
                ev[0].record()
                R._prepare(cat, first, N, 4, 2, 5, 224, 4)
                ev[1].record()
                ev[1].synchronize()
                phases["prepare"] = phases.get("prepare", 0.0) + ev[0].elapsed_time(ev[1])
                pooler(x, boxes, _phase_ms=phases).backward(g)
            torch.cuda.synchronize()
            t_fwd, t_bwd = timed(lambda: _torch_ops_pool(x, cat, levels, P, first), max(args.iters // 4, 2), 1)
            esize = 2 if dtype == torch.bfloat16 else 4
            bytes_fwd = esize * (rows * C * P * P + touched * C)
            bytes_bwd = esize * (rows * C * P * P + map_elements)
            cases[f"P{P}_{'bf16' if esize == 2 else 'f32'}"] = {
                "forward_ms": fwd_ms, "backward_ms": bwd_ms, "kernels_ms": {k: round(v / args.iters, 4) for k, v in phases.items()},
                "bytes": {"forward": bytes_fwd, "backward": bytes_bwd},
                "floor_ms": {"forward": round(bytes_fwd / (args.hbm_tbs * 1e9), 4), "backward": round(bytes_bwd / (args.hbm_tbs * 1e9), 4)},
                "ratio2_ms": {"forward": r2_fwd, "backward": r2_bwd}, "torch_ops_ms": {"forward": t_fwd, "backward": t_bwd}}
            del x, g
    line = {"tool": "roi_pool_bench", "images": N, "hw": list(FRAME), "strides": list(STRIDES), "channels": C, "proposals_per_image": PER_IMAGE,
            "boxes_per_level": np.bincount(np.concatenate(levels_np), minlength=4).tolist(), "iters": args.iters, "warmup": args.warmup,
            "hbm_tbs": args.hbm_tbs, "cases": cases, "host_procs": args.procs, "host_ms_P7_f32": None if host_ms is None else round(host_ms, 1),
            "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
