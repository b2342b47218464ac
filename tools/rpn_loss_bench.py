"""The RPN's training half on the device (unmore_amd.rpn_loss: label_and_sample_anchors + rpn_losses) beside the torch-ops composition
of the same steps and the NumPy restatement: one JSON line per dtype, appended to profiles/rpn_loss_bench.jsonl.

    python tools/rpn_loss_bench.py --images 16 --iters 20 --warmup 5

The workload is the recipe's: `--images` frames of 800x1216, p2..p6 (strides 4..64), A = 3 anchors of sizes 32..512 x (0.5, 1, 2), 20
seeded ground truths per image, thresholds (0.3, 0.7) with low-quality matches, B = 256 at fraction 0.5, smooth-L1 at beta 0.
  label_call_ms:    a host clock around label_and_sample_anchors (checks, one torch.cat and one small upload, the three launches), median.
  loss_call_ms:     a host clock around rpn_losses and the backward of the sum of both losses (the zeroing of the gradient maps, one small
                    upload, two launches; the backward scales the saved maps), median.
  launch_ms:        device events around each launch alone (match, label, partial_select, select; terms, sum).
  launch_bytes:     what each launch must move at least: match writes 8 bytes per (image, anchor); label reads 4 and writes 1;
                    partial_select reads the image's labels once from memory (the two classes' five passes find them in L2) and writes
                    its survivors, at most 4 bytes per (part, batch slot); select reads those and writes 8 bytes per sample;
                    terms reads 8 bytes per sample, one logit and (positives) four deltas, and writes as many gradient elements; sum reads
                    24 bytes per image.  zero_maps: the gradient maps the call zeroes, 5 A elements per position.  floor_us: their sum
                    at `--hbm-gbps`.
  torch_ms:         the torch ops of Detectron2's label_and_sample_anchors and losses on the GPU with their backward, host clock, median:
                    per image the [G, R] IoU matrix, two max, the equality mask and its nonzero, two nonzero and two randperm, the stack
                    of matched boxes, get_deltas on every anchor; the two .item() reads of the logged counts.
  numpy_ms:         the NumPy restatement (tests/rpn_loss_common.py) of both calls, images spread over `--procs` processes, one run."""
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

H, W, A, G, B, FRACTION = 800, 1216, 3, 20, 256, 0.5
STRIDES = (4, 8, 16, 32, 64)
SIZES = ((32,), (64,), (128,), (256,), (512,))
RATIOS = (0.5, 1.0, 2.0)


def _maps():
    return [(-(-H // s), -(-W // s)) for s in STRIDES]


def _ground_truths(N, seed):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(N):
        side = np.exp(rng.uniform(np.log(24.0), np.log(0.8 * H), G))
        aspect = np.exp(rng.uniform(np.log(0.5), np.log(2.0), G))
        bw, bh = np.minimum(side / np.sqrt(aspect), W), np.minimum(side * np.sqrt(aspect), H)
        x1, y1 = rng.uniform(0, 1, G) * (W - bw), rng.uniform(0, 1, G) * (H - bh)
        out.append(np.stack([x1, y1, x1 + bw, y1 + bh], axis=1).astype(np.float32))
    return out


def _numpy_image(args):
    import rpn_loss_common as C
    logits, deltas, cells, gt, n, seed = args
    maps = [tuple(x.shape[2:]) for x in logits]
    r = C.label_and_sample_np(cells, STRIDES, maps, [gt], [(H, W)], B, FRACTION, seed=seed)[0]
    # the hash takes the image's index: image n of the batch is image 0 here, so only the counts are compared with the device
    out = C.losses_np(logits, deltas, [(r["pos"], r["neg"], r["gt"])], cells, STRIDES, [gt], B)
    return r["counters"].tolist(), float(out[0]), float(out[1])


def _median_ms(fn, iters, warmup, sync):
    times = []
    for i in range(warmup + iters):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), out


def _torch_step(logits, deltas, anchors, gts):
    """Detectron2's label_and_sample_anchors + losses in torch ops, with the backward"""
    import torch
    import torch.nn.functional as F
    N = logits[0].shape[0]
    R = anchors.shape[0]
    a_area = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    labels_all, matched = [], []
    for gt in gts:
        g_area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
        wh = (torch.min(gt[:, None, 2:], anchors[:, 2:]) - torch.max(gt[:, None, :2], anchors[:, :2])).clamp_(min=0)
        inter = wh.prod(dim=2)
        m = torch.where(inter > 0, inter / (g_area[:, None] + a_area - inter), torch.zeros(1, dtype=inter.dtype, device=inter.device))
        vals, idx = m.max(dim=0)
        labels = torch.full((R,), 1, dtype=torch.int8, device=m.device)
        labels[vals < 0.3] = 0
        labels[(vals >= 0.3) & (vals < 0.7)] = -1
        row_max, _ = m.max(dim=1)
        labels[(m == row_max[:, None]).nonzero()[:, 1]] = 1
        positive, negative = (labels == 1).nonzero().squeeze(1), (labels == 0).nonzero().squeeze(1)
        num_pos = min(positive.numel(), int(B * FRACTION))
        num_neg = min(negative.numel(), B - num_pos)
        pos_idx = positive[torch.randperm(positive.numel(), device=m.device)[:num_pos]]
        neg_idx = negative[torch.randperm(negative.numel(), device=m.device)[:num_neg]]
        labels.fill_(-1)
        labels[pos_idx], labels[neg_idx] = 1, 0
        labels_all.append(labels)
        matched.append(gt[idx])
    labels = torch.stack(labels_all)
    pos_mask, valid = labels == 1, labels >= 0
    logged = (pos_mask.sum().item(), (labels == 0).sum().item())
    lg = [x.detach().requires_grad_(True) for x in logits]
    dl = [x.detach().requires_grad_(True) for x in deltas]
    flat_l = torch.cat([x.permute(0, 2, 3, 1).flatten(1) for x in lg], dim=1).float()
    flat_d = torch.cat([x.view(N, A, 4, x.shape[2], x.shape[3]).permute(0, 3, 4, 1, 2).flatten(1, -2) for x in dl], dim=1).float()
    sw, sh = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    scx, scy = anchors[:, 0] + 0.5 * sw, anchors[:, 1] + 0.5 * sh
    targets = []
    for t in matched:
        tw, th = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
        tcx, tcy = t[:, 0] + 0.5 * tw, t[:, 1] + 0.5 * th
        targets.append(torch.stack(((tcx - scx) / sw, (tcy - scy) / sh, torch.log(tw / sw), torch.log(th / sh)), dim=1))
    loc = (flat_d[pos_mask] - torch.stack(targets)[pos_mask]).abs().sum() / (B * N)
    cls = F.binary_cross_entropy_with_logits(flat_l[valid], labels[valid].float(), reduction="sum") / (B * N)
    (cls + loc).backward()
    return cls.detach(), loc.detach(), logged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpn_loss_bench.jsonl"))
    args = ap.parse_args()
    args.procs = max(1, min(args.procs, 16))
    pool = None
    if not args.skip_numpy:
        pool = multiprocessing.get_context("spawn").Pool(args.procs)          # fresh processes that never open the GPU, before this one does
        pool.map(abs, range(args.procs))
    import torch
    from unmore_amd import rpn, rpn_loss
    assert torch.cuda.is_available(), "rpn_loss_bench needs the MI355X"
    dev = torch.device("cuda:0")
    N = args.images
    sync = torch.cuda.synchronize
    cells = rpn.cell_anchors(SIZES, RATIOS)
    maps = _maps()
    R = sum(h * w for h, w in maps) * A
    sizes = [(H, W)] * N
    gts_np = _ground_truths(N, args.seed)
    gts = [torch.from_numpy(g).to(dev) for g in gts_np]
    anchors = torch.cat([a.to(dev) for a in rpn.grid_anchors(cells, STRIDES, maps)])
    gen = torch.Generator().manual_seed(args.seed)
    base_logits = [torch.randn((N, A, h, w), generator=gen) for h, w in maps]
    base_deltas = [torch.randn((N, 4 * A, h, w), generator=gen) * 0.2 for h, w in maps]
    for dtype in (torch.float32, torch.bfloat16):
        lg = [x.to(dev).to(dtype).contiguous().requires_grad_(True) for x in base_logits]
        dl = [x.to(dev).to(dtype).contiguous().requires_grad_(True) for x in base_deltas]
        esize = lg[0].element_size()
        label = lambda **kw: rpn_loss.label_and_sample_anchors(cells, STRIDES, maps, gts, sizes, batch_size_per_image=B,       # noqa: E731
                                                               positive_fraction=FRACTION, seed=args.seed, **kw)

        def loss(s, **kw):
            for t in lg + dl:
                t.grad = None
            out = rpn_loss.rpn_losses(lg, dl, s, cells, STRIDES, gts, batch_size_per_image=B, **kw)
            (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()
            return out
        label_ms, samples = _median_ms(label, args.iters, args.warmup, sync)
        loss_ms, out = _median_ms(lambda: loss(samples), args.iters, args.warmup, sync)
        phases, st = {}, {}
        for _ in range(args.iters):
            s = label(stats=st, _phase_ms=phases)
            loss(s, _phase_ms=phases)
        counters = st["counters"].cpu().numpy()
        n_samples, n_pos = int(counters[:, 2:4].sum()), int(counters[:, 2].sum())
        survivors = N * -(-R // rpn_loss.SELECT_SHARE) * B * 4                      # an upper bound: a part leaves at most its class's share
        nbytes = {"match": N * R * 8, "label": N * R * 5, "partial_select": N * R + survivors, "select": survivors + n_samples * 8,
                  "terms": n_samples * (8 + 2 * esize) + n_pos * (16 + 8 * esize), "sum": N * 24, "zero_maps": N * R * 5 * esize}
        torch_ms, tout = _median_ms(lambda: _torch_step(lg, dl, anchors, gts), args.iters, args.warmup, sync)
        numpy_ms = None
        if pool is not None:
            wl = [x.detach().float().cpu().numpy() for x in lg]
            wd = [x.detach().float().cpu().numpy() for x in dl]
            cn = [c.numpy() for c in cells]
            t0 = time.perf_counter()
            res = pool.map(_numpy_image, [([x[n:n + 1] for x in wl], [x[n:n + 1] for x in wd], cn, gts_np[n], n, args.seed) for n in range(N)])
            numpy_ms = (time.perf_counter() - t0) * 1e3
            same = [r[0] == counters[n].tolist() for n, r in enumerate(res)]
            print(f"# numpy restatement: {sum(same)} of {N} images have the device's counters", file=sys.stderr)
        line = {"tool": "rpn_loss_bench", "images": N, "frame_hw": [H, W], "levels": maps, "anchors": A, "anchors_per_image": R,
                "gt_per_image": G, "batch_size_per_image": B, "dtype": str(dtype).replace("torch.", ""), "iters": args.iters,
                "warmup": args.warmup, "label_call_ms": round(label_ms, 4), "loss_call_ms": round(loss_ms, 4),
                "call_ms": round(label_ms + loss_ms, 4), "launch_ms": {k: round(v / args.iters, 4) for k, v in phases.items()},
                "launches_ms": round(sum(phases.values()) / args.iters, 4), "launch_bytes": nbytes,
                "floor_us": round(sum(nbytes.values()) / (args.hbm_gbps * 1e9) * 1e6, 2), "hbm_gbps": args.hbm_gbps,
                "torch_ms": round(torch_ms, 4), "numpy_ms": None if numpy_ms is None else round(numpy_ms, 1),
                "numpy_procs": args.procs if pool is not None else 0, "positives": int(counters[:, 0].sum()),
                "negatives": int(counters[:, 1].sum()), "sampled_positives": n_pos, "sampled_negatives": n_samples - n_pos,
                "loss_rpn_cls": float(out["loss_rpn_cls"].detach()), "loss_rpn_loc": float(out["loss_rpn_loc"].detach()),
                "torch_loss_rpn_cls": float(tout[0]), "torch_loss_rpn_loc": float(tout[1]),
                "device_name": torch.cuda.get_device_name(0)}
        print(json.dumps(line))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == "__main__":
    main()
