"""The RPN's proposal step on the device (unmore_amd.rpn.rpn_proposals) beside the torch-ops composition of its pre-NMS half and the
NumPy restatement: one JSON line per (recipe setting, dtype), appended to profiles/rpn_proposals_bench.jsonl.

    python tools/rpn_bench.py --images 16 --iters 20 --warmup 5

The workload is the recipe's: `--images` frames of 800x1216, p2..p6 (strides 4..64), A = 3 anchors of sizes 32..512 x (0.5, 1, 2), NMS at
0.65, in both settings -- training (pre 2000 / post 4000) and inference (1000 / 1000) -- and both dtypes.  The logits are a seeded smooth
field plus noise, so that the top scores cluster and the NMS has work; the deltas are normal x 0.2.
  call_ms:          a host clock around rpn_proposals (checks, one small upload, the launches, the one read of the counts), median; and
                    the padded form, which reads nothing back.
  launch_ms:        device events around each launch alone (partial_select, select, suppression, scan, merge).
  launch_bytes:     what each launch must move at least: partial_select reads every score of the levels above SELECT_SHARE once and
                    writes its survivors (8 bytes each); select reads the other levels' scores and those survivors once, four deltas
                    and the logit per candidate, and writes 25 bytes per candidate; suppression reads 16 bytes per candidate and writes
                    the upper triangle of the bit matrices; scan reads the rows of the kept candidates (the upper triangle's share) and
                    moves 20 bytes per kept box; merge moves 20 bytes per kept box in and per output row out.  floor_us: their sum at
                    `--hbm-gbps`.
  torch_pre_nms_ms: the torch ops of the reference's pre-NMS half on the GPU, host clock, median: per level permute + flatten of the logits
                    and deltas, the decode of ALL anchors, topk, gather; per image isfinite, clip, the non-empty mask.  Its NMS half
                    (torchvision's batched_nms) has no counterpart here and is NOT in the number.
  numpy_ms:         the NumPy restatement (tests/rpn_common.py) of the whole step, images spread over `--procs` processes, one run."""
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

H, W, A, THRESH = 800, 1216, 3, 0.65
STRIDES = (4, 8, 16, 32, 64)
SIZES = ((32,), (64,), (128,), (256,), (512,))
RATIOS = (0.5, 1.0, 2.0)
SETTINGS = {"train": (2000, 4000), "test": (1000, 1000)}


def _maps():
    return [(-(-H // s), -(-W // s)) for s in STRIDES]


def _numpy_images(args):
    import rpn_common as C
    logits, deltas, cells, sizes, pre, post = args
    return [(len(r["boxes"]), r["counters"].tolist()) for r in C.proposals_np(logits, deltas, cells, STRIDES, sizes, THRESH, pre, post)]


def _inputs(N, seed):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    logits, deltas = [], []
    for h, w in _maps():
        low = torch.randn((N, A, max(h // 8, 2), max(w // 8, 2)), generator=g) * 2
        logits.append((F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False) + torch.randn((N, A, h, w), generator=g) * 0.3)
                      .contiguous())
        deltas.append(torch.randn((N, 4 * A, h, w), generator=g) * 0.2)
    return logits, deltas


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


def _torch_pre_nms(logits, deltas, anchors, sizes, pre):
    import torch
    N = logits[0].shape[0]
    clamp = float(np.log(1000.0 / 16.0))
    batch = torch.arange(N, device=logits[0].device)[:, None]
    boxes, scores = [], []
    for s, d, an in zip(logits, deltas, anchors):
        _, _, h, w = s.shape
        sc = s.permute(0, 2, 3, 1).flatten(1).float()
        dl = d.view(N, A, 4, h, w).permute(0, 3, 4, 1, 2).flatten(1, -2).float().reshape(-1, 4)
        a = an.unsqueeze(0).expand(N, -1, -1).reshape(-1, 4)
        ws, hs = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cx, cy = a[:, 0] + 0.5 * ws, a[:, 1] + 0.5 * hs
        dw, dh = torch.clamp(dl[:, 2], max=clamp), torch.clamp(dl[:, 3], max=clamp)
        pcx, pcy = dl[:, 0] * ws + cx, dl[:, 1] * hs + cy
        pw, ph = torch.exp(dw) * ws, torch.exp(dh) * hs
        prop = torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1).view(N, -1, 4)
        top, idx = sc.topk(min(pre, sc.shape[1]), dim=1)
        boxes.append(prop[batch, idx])
        scores.append(top)
    boxes, scores = torch.cat(boxes, dim=1), torch.cat(scores, dim=1)
    out = []
    for n, (ih, iw) in enumerate(sizes):
        b, s = boxes[n], scores[n]
        ok = torch.isfinite(b).all(dim=1) & torch.isfinite(s)
        b = torch.stack((b[:, 0].clamp(0, iw), b[:, 1].clamp(0, ih), b[:, 2].clamp(0, iw), b[:, 3].clamp(0, ih)), dim=1)
        ok = ok & ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        out.append((b, s, ok))
    return out


def _bytes(N, pre, esize, counters, proposals, share):
    """the least each launch moves, from the shapes and the call's own counters [N, L, 5]"""
    ns = [h * w * A for h, w in _maps()]
    ks = [min(n, pre) for n in ns]
    big = [n > share for n in ns]
    part_len = [((n + share - 1) // share - 1) * k + min(k, n - ((n + share - 1) // share - 1) * share) if b else 0
                for n, k, b in zip(ns, ks, big)]
    cand, kept = N * sum(ks), int(counters[:, :, 4].sum())
    tri = [k * ((k + 63) // 64) * 8 // 2 for k in ks]
    kept_rows = sum(int(counters[:, l, 4].sum()) * ((k + 63) // 64) * 8 // 2 for l, k in enumerate(ks))
    return {"partial_select": N * sum(n * esize + p * 8 for n, p, b in zip(ns, part_len, big) if b),
            "select": N * sum((0 if b else n * esize) + p * 8 for n, p, b in zip(ns, part_len, big)) + cand * (5 * esize + 25),
            "suppression": cand * 16 + N * sum(tri), "scan": kept_rows + kept * 40, "merge": kept * 20 + proposals * 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpn_proposals_bench.jsonl"))
    args = ap.parse_args()
    args.procs = max(1, min(args.procs, 16))
    pool = None
    if not args.skip_numpy:
        pool = multiprocessing.get_context("spawn").Pool(args.procs)          # fresh processes that never open the GPU, before this one does
        pool.map(abs, range(args.procs))
    import torch
    from unmore_amd import rpn
    assert torch.cuda.is_available(), "rpn_bench needs the MI355X"
    dev = torch.device("cuda:0")
    N = args.images
    sync = torch.cuda.synchronize
    cells = rpn.cell_anchors(SIZES, RATIOS)
    sizes = [(H, W)] * N
    base_logits, base_deltas = _inputs(N, args.seed)
    anchors = [a.to(dev) for a in rpn.grid_anchors(cells, STRIDES, _maps())]
    for dtype in (torch.float32, torch.bfloat16):
        lg = [x.to(dev).to(dtype).contiguous() for x in base_logits]
        dl = [x.to(dev).to(dtype).contiguous() for x in base_deltas]
        for name, (pre, post) in SETTINGS.items():
            kw = {"nms_thresh": THRESH, "pre_nms_topk": pre, "post_nms_topk": post}
            call_ms, out = _median_ms(lambda: rpn.rpn_proposals(lg, dl, cells, STRIDES, sizes, **kw), args.iters, args.warmup, sync)
            padded_ms, _ = _median_ms(lambda: rpn.rpn_proposals(lg, dl, cells, STRIDES, sizes, padded=True, **kw), args.iters, args.warmup, sync)
            phases, st = {}, {}
            for _ in range(args.iters):
                rpn.rpn_proposals(lg, dl, cells, STRIDES, sizes, padded=True, stats=st, _phase_ms=phases, **kw)
            counters = st["counters"].cpu().numpy()
            torch_ms, _ = _median_ms(lambda: _torch_pre_nms(lg, dl, anchors, sizes, pre), args.iters, args.warmup, sync)
            nbytes = _bytes(N, pre, lg[0].element_size(), counters, int(sum(len(s) for _, s in out)), rpn.SELECT_SHARE)
            numpy_ms = None
            if pool is not None:
                wl = [x.float().cpu().numpy() for x in lg]
                wd = [x.float().cpu().numpy() for x in dl]
                cn = [c.numpy() for c in cells]
                t0 = time.perf_counter()
                res = pool.map(_numpy_images, [([x[n:n + 1] for x in wl], [x[n:n + 1] for x in wd], cn, sizes[n:n + 1], pre, post)
                                               for n in range(N)])
                numpy_ms = (time.perf_counter() - t0) * 1e3
                same = [r[0][0] == len(o[1]) for r, o in zip(res, out)]
                print(f"# numpy restatement: {sum(same)} of {N} images keep the same number of proposals as the device "
                      "(a last bit of expf may move one)", file=sys.stderr)
            line = {"tool": "rpn_bench", "images": N, "frame_hw": [H, W], "levels": _maps(), "anchors": A, "setting": name,
                    "pre_nms_topk": pre, "post_nms_topk": post, "nms_thresh": THRESH, "dtype": str(dtype).replace("torch.", ""),
                    "iters": args.iters, "warmup": args.warmup, "call_ms": round(call_ms, 4), "padded_call_ms": round(padded_ms, 4),
                    "launch_ms": {k: round(v / args.iters, 4) for k, v in phases.items()},
                    "launches_ms": round(sum(phases.values()) / args.iters, 4), "launch_bytes": nbytes,
                    "floor_us": round(sum(nbytes.values()) / (args.hbm_gbps * 1e9) * 1e6, 2), "hbm_gbps": args.hbm_gbps,
                    "torch_pre_nms_ms": round(torch_ms, 4), "numpy_ms": None if numpy_ms is None else round(numpy_ms, 1),
                    "numpy_procs": args.procs if pool is not None else 0,
                    "candidates": int(counters[:, :, 0].sum()), "suppressed": int(counters[:, :, 3].sum()), "kept": int(counters[:, :, 4].sum()),
                    "proposals": int(sum(len(s) for _, s in out)), "device_name": torch.cuda.get_device_name(0)}
            print(json.dumps(line))
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == "__main__":
    main()
