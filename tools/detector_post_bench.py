"""The detector's inference tail on the device (unmore_amd.detector_inference: select_detections, then coco_records) beside its unfused
form and the host way: one JSON line per run, appended to profiles/detector_post_bench.jsonl.

    python tools/detector_post_bench.py --images 16 --iters 20 --warmup 5

The input is a seeded batch of `--images` network frames of 800x1216 with 1000 proposals each (boxes scattered around 30 objects, the
recipe's one class, class-agnostic boxes, score threshold 0, NMS at 0.5, top 100), original frames of 480x640 and blob-shaped 28x28 mask
logits for the kept detections.
  select_ms:        a host clock around select_detections (checks, table upload, three launches) ending in a synchronise, median.
  select_kernels_ms: device events around the three launches alone, after the table is up: candidates + ranks, suppression matrix, scan.
  records_ms:       three arms that produce the same records from the same detections, host clock, median:
                      fused     coco_records: scale + clip, the measure pass and the write pass straight from the logits, four small reads
                      unfused   the same boxes, paste_masks into uint8 frames on the device, rle.encode of the frames
                      host      the frames to the host, rle.encode_numpy on `--procs` processes (the reference encodes one by one)
                    The three arms' records are compared; `records_equal` says so.
  rle_kernels_ms:   device events around the measure and the write launch of the fused arm."""
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

H, W, OUT_H, OUT_W, PER_IMAGE, OBJECTS, TOPK, M = 800, 1216, 480, 640, 1000, 30, 100, 28


def _encode_chunk(frames):
    from unmore_amd import rle
    return [rle.encode_numpy(f) for f in frames]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detector_post_bench.jsonl"))
    args = ap.parse_args()
    args.procs = max(1, min(args.procs, 16))
    pool = multiprocessing.get_context("spawn").Pool(args.procs)              # fresh processes that never open the GPU, before this one does
    pool.map(_encode_chunk, [[np.zeros((2, 2), np.uint8)]] * args.procs)
    import torch
    from det_post_common import blob_logits
    from unmore_amd import detector_inference as D
    from unmore_amd import rle
    assert torch.cuda.is_available(), "detector_post_bench needs the MI355X"
    dev = torch.device("cuda:0")
    N = args.images
    rng = np.random.RandomState(args.seed)
    boxes, scores = [], []
    for _ in range(N):
        centres = rng.uniform(0.1, 0.9, (OBJECTS, 2)) * [W, H]
        sizes = rng.uniform(0.08, 0.35, (OBJECTS, 2)) * [W, H]
        which = rng.randint(OBJECTS, size=PER_IMAGE)
        c = centres[which] + rng.normal(0, 0.08, (PER_IMAGE, 2)) * sizes[which]
        s = sizes[which] * rng.uniform(0.85, 1.15, (PER_IMAGE, 2))
        boxes.append(np.concatenate([c - s / 2, c + s / 2], axis=1).astype(np.float32))
        p = rng.uniform(0, 1, PER_IMAGE).astype(np.float32)
        scores.append(np.stack([p, 1 - p], axis=1))
    d_boxes, d_scores = [torch.from_numpy(b).to(dev) for b in boxes], [torch.from_numpy(s).to(dev) for s in scores]
    shapes, out_sizes, ids = [(H, W)] * N, [(OUT_H, OUT_W)] * N, list(range(N))
    sync = torch.cuda.synchronize

    select_ms, sel = _median_ms(lambda: D.select_detections(d_boxes, d_scores, shapes, 0.0, 0.5, TOPK), args.iters, args.warmup, sync)
    phases = {}
    for _ in range(args.iters):
        D.select_detections(d_boxes, d_scores, shapes, 0.0, 0.5, TOPK, _phase_ms=phases)
    dets, _ = D.split_detections(sel)
    counts = [len(d["scores"]) for d in dets]
    n = sum(counts)
    logits = torch.from_numpy(blob_logits(rng, n, 1, M)).to(dev)

    fused_ms, fused = _median_ms(lambda: D.coco_records(dets, logits, shapes, out_sizes, ids), args.iters, args.warmup, sync)
    rle_phases = {}
    for _ in range(args.iters):
        D.coco_records(dets, logits, shapes, out_sizes, ids, _phase_ms=rle_phases)
    bare = D.coco_records(dets, None, shapes, out_sizes, ids)                 # the scaled boxes both other arms paste into
    sx, sy = D.scale_ratio(OUT_W, W), D.scale_ratio(OUT_H, H)
    scale = torch.tensor([sx, sy, sx, sy], dtype=torch.float32, device=dev)
    hi = torch.tensor([OUT_W, OUT_H, OUT_W, OUT_H], dtype=torch.float32, device=dev)

    def frames_of(k):
        b = torch.minimum(torch.clamp(dets[k]["pred_boxes"] * scale, min=0), hi)
        keep = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        at = sum(counts[:k])
        return D.paste_masks(logits[at:at + counts[k]][keep], b[keep], None, OUT_H, OUT_W)

    def unfused():
        return [rle.encode(frames_of(k)) if counts[k] else [] for k in range(N)]

    def host():
        out = []
        for k in range(N):
            f = frames_of(k).cpu().numpy()
            parts = pool.map(_encode_chunk, [f[i::args.procs] for i in range(args.procs)])
            mine = [None] * len(f)
            for i, part in enumerate(parts):
                mine[i::args.procs] = part
            out.append(mine)
        return out

    unfused_ms, unf = _median_ms(unfused, args.iters, args.warmup, sync)
    host_ms, hst = _median_ms(host, args.host_iters, 1, sync)
    pool.close()
    pool.join()
    equal = all(len(f) == len(u) == len(h) == len(b) and all(r["segmentation"] == x == y for r, x, y in zip(f, u, h))
                for f, u, h, b in zip(fused, unf, hst, bare))
    assert equal, "the three arms' records differ"
    chars = sum(len(r["segmentation"]["counts"]) for f in fused for r in f)
    area = sum(rle.area(r["segmentation"]) for f in fused for r in f)
    line = {"tool": "detector_post_bench", "images": N, "network_hw": [H, W], "output_hw": [OUT_H, OUT_W], "proposals_per_image": PER_IMAGE,
            "topk": TOPK, "mask_side": M, "kept": n, "records": sum(len(f) for f in fused), "iters": args.iters, "warmup": args.warmup,
            "select_ms": round(select_ms, 4), "select_kernels_ms": {k: round(v / args.iters, 4) for k, v in phases.items()},
            "records_ms": {"fused": round(fused_ms, 3), "unfused": round(unfused_ms, 3), "host": round(host_ms, 1)},
            "rle_kernels_ms": {k: round(v / args.iters, 4) for k, v in rle_phases.items()}, "records_equal": equal,
            "string_chars": chars, "mask_pixels_set": int(area), "host_procs": args.procs, "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
