"""Polygon segmentations -> COCO run-length records on the device (unmore_amd.rle.from_polygons) beside the sequential restatement the
tests compare it against (rle.from_polygons_numpy): one JSON line per run, appended to profiles/polygon_rle_bench.jsonl.

    python tools/polygon_rle_bench.py --annotations 5000 --iters 5 --warmup 2

The input is a seeded set of annotations on 640x480 images: ellipse-like outlines of 20-120 vertices, one annotation in five made of 2-4
polygons -- the shape of COCO's own ground truths, which is what the evaluator's polygons="rasterize" converts.
  device_annotations_per_s: the whole call -- host checks and tables, one upload, the three phases, the two read-backs, the records as
                            Python dicts -- as a host clock around it, median of `--iters`.
  kernels_ms:               device events around the phases: generate (outline points -> column crossings), sort (per polygon and per
                            annotation), characters (measure pass + write pass of the run-length back end).
  host_annotations_per_s:   from_polygons_numpy over the same annotations spread over `--procs` worker processes.  It stands in for
                            pycocotools' annToRLE, which is not a dependency here; pycocotools' C loops are much faster than these.
The two give the same records (`equal_to_restatement`)."""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

H, W = 480, 640


def make_annotations(n, seed=0):
    rng = np.random.default_rng(seed)
    segs = []
    for i in range(n):
        seg = []
        for _ in range(int(rng.integers(2, 5)) if i % 5 == 4 else 1):
            k = int(rng.integers(20, 121))
            t = np.arange(k) * 2 * np.pi / k
            cx, cy, rx, ry = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(5, 160), rng.uniform(5, 120)
            r = rng.uniform(0.85, 1.0, k)
            pts = np.stack([cx + rx * r * np.cos(t), cy + ry * r * np.sin(t)], axis=1)
            seg.append([float(v) for v in np.round(pts.reshape(-1), 2)])        # COCO stores two decimals
        segs.append(seg)
    return segs


def host_chunk(segs):
    from unmore_amd import rle
    return rle.from_polygons_numpy(segs, (H, W))


def host_arm(segs, procs):
    chunks = [segs[i:i + 25] for i in range(0, len(segs), 25)]
    with multiprocessing.get_context("spawn").Pool(procs) as pool:
        pool.map(host_chunk, [c[:1] for c in chunks[:procs]])          # the workers' imports are not timed
        t0 = time.perf_counter()
        out = pool.map(host_chunk, chunks, chunksize=1)
        dt = time.perf_counter() - t0
    return [r for c in out for r in c], len(segs) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--annotations", type=int, default=5000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16, help="worker processes of the host arm")
    ap.add_argument("--no-host", action="store_true", help="skip the restatement arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygon_rle_bench.jsonl"))
    a = ap.parse_args()
    segs = make_annotations(a.annotations)
    rec = {"tool": "polygon_rle_bench", "annotations": a.annotations, "polygons": sum(len(s) for s in segs),
           "vertices": sum(len(p) // 2 for s in segs for p in s), "hw": [H, W], "iters": a.iters, "warmup": a.warmup, "host_procs": a.procs}
    want = None
    if not a.no_host:                                       # before this process opens the GPU: the workers never do
        want, rec["host_annotations_per_s"] = host_arm(segs, a.procs)
        rec["host_annotations_per_s"] = round(rec["host_annotations_per_s"], 1)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("polygon_rle_bench measures on the MI355X; no GPU found")
    from unmore_amd import rle
    wall, phases = [], []
    for it in range(a.warmup + a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = rle.from_polygons(segs, (H, W))
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    for it in range(a.warmup + a.iters):                    # the phases in a run of their own: the events synchronise between them
        ms = {}
        rle.from_polygons(segs, (H, W), phase_ms=ms)
        phases.append(ms)
    rec["device_annotations_per_s"] = round(a.annotations / statistics.median(wall[a.warmup:]), 1)
    rec["device_ms"] = round(statistics.median(wall[a.warmup:]) * 1e3, 3)
    rec["kernels_ms"] = {k: round(statistics.median(p[k] for p in phases[a.warmup:]), 4) for k in ("generate", "sort", "characters")}
    rec["characters_total"] = sum(len(r["counts"]) for r in got)
    if want is not None:
        rec["equal_to_restatement"] = got == want
        rec["device_over_host"] = round(rec["device_annotations_per_s"] / rec["host_annotations_per_s"], 1)
    rec["device_name"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    if want is not None and got != want:
        raise SystemExit("the device rasteriser and the restatement disagree")


if __name__ == "__main__":
    main()
