"""COCO AP / AR evaluation on the device (unmore_amd.coco_eval.COCOEvaluator) beside the plain numpy restatement the tests compare it
against: one JSON line per run, appended to profiles/coco_eval_bench.jsonl.

    python tools/coco_eval_bench.py --images 16 --iters 5 --warmup 2

Every image is 640x480 with 20 ground-truth blobs and 100 detections (jittered copies of the ground truths plus noise blobs), one
category.  Per task (segm, bbox):
  device_ms_per_image:  COCOEvaluator.evaluate() for that task alone -- host tables, uploads, the IoU and matching launches, the read-back
                        of the match tables, accumulate and summarize on the host -- as a host clock around the call, median of `--iters`.
  kernels_ms_per_image: device events around the library calls inside it: iou (umr_mask_iou: parse + bit planes + AND/popcount tiles, or
                        umr_box_iou) and match (umr_coco_match).
  host_ms_per_image:    the restatement (tests/coco_eval_common.py: dense masks, Python loops) over the same data, images spread over
                        `--procs` worker processes, IoU and matching only (its accumulate is not counted).  It stands in for pycocotools,
                        which is not a dependency here; pycocotools' C loops are much faster than these.
The two give the same twelve statistics at the sizes timed (`equal_to_restatement`)."""
import argparse
import json
import math
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

H, W, N_GT, N_DT = 480, 640, 20, 100


def make_scene(n_images, seed=0):
    from coco_eval_common import blob, dataset, dt_ann, gt_ann
    rng = np.random.default_rng(seed)
    anns, dts, images, aid = [], [], [], 1
    for img in range(1, n_images + 1):
        images.append((img, H, W))
        shapes = []
        for k in range(N_GT):
            s = (rng.uniform(20, H - 20), rng.uniform(20, W - 20), rng.uniform(4, 90), rng.uniform(4, 120))
            shapes.append(s)
            anns.append(gt_ann(aid, img, blob(H, W, *s), iscrowd=int(k == N_GT - 1)))
            aid += 1
        for k in range(N_DT):
            if k < 3 * N_GT:
                j = rng.normal(0, 3.0 * (1 + k // N_GT), 4)
                cy, cx, ry, rx = shapes[k % N_GT]
                m = blob(H, W, cy + j[0], cx + j[1], ry + j[2], rx + j[3])
            else:
                m = blob(H, W, rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, 60), rng.uniform(2, 60))
            dts.append(dt_ann(img, m, float(np.round(rng.random(), 3))))
    return dataset(images, anns), dts


def host_image(job):
    """the restatement's computeIoU + evaluateImg for one image"""
    from coco_eval_common import AREA_RNG, IOU_THRS, Restatement, evaluate_img
    gt, dts, task, img = job
    r = Restatement(gt, dts, task)
    ious, dt, g = r.compute_iou(img, 1)
    return [evaluate_img(ious, [float(d["score"]) for d in dt], [d["area"] for d in dt], [x["area"] for x in g],
                         [int(x.get("iscrowd", 0)) for x in g], rng, IOU_THRS, 100)["dtm"].sum() for rng in AREA_RNG]


def host_arm(gt, dts, task, procs):
    jobs = []
    for im in gt["images"]:
        sub = {"images": [im], "annotations": [a for a in gt["annotations"] if a["image_id"] == im["id"]], "categories": gt["categories"]}
        jobs.append((sub, [d for d in dts if d["image_id"] == im["id"]], task, im["id"]))
    with multiprocessing.get_context("spawn").Pool(procs) as pool:
        pool.map(host_image, jobs[:procs])                # the workers' imports are not timed
        t0 = time.perf_counter()
        pool.map(host_image, jobs, chunksize=1)
        return (time.perf_counter() - t0) * 1e3 / len(jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16, help="worker processes of the host arm")
    ap.add_argument("--no-host", action="store_true", help="skip the restatement arm (it is slow)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_bench.jsonl"))
    a = ap.parse_args()
    gt, dts = make_scene(a.images)
    rec = {"tool": "coco_eval_bench", "images": a.images, "hw": [H, W], "detections_per_image": N_DT, "ground_truths_per_image": N_GT,
           "iters": a.iters, "warmup": a.warmup, "host_procs": a.procs}
    host = {}
    if not a.no_host:                                       # before this process opens the GPU: the workers never do
        for task in ("segm", "bbox"):
            host[task] = host_arm(gt, dts, task, a.procs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_bench measures on the MI355X; no GPU found")
    from unmore_amd import _lib, coco_eval
    from coco_eval_common import METRICS, Restatement
    lib = _lib.lib()
    spans = []

    def timed(name):
        fn = getattr(lib, name)

        def call(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args)
            e1.record()
            spans.append((name, e0, e1))
            return r
        setattr(lib, name, call)
    for name in ("umr_mask_iou", "umr_box_iou", "umr_coco_match"):
        timed(name)
    by = {}
    for d in dts:
        by.setdefault(d["image_id"], []).append(d)
    equal = True
    for task in ("segm", "bbox"):
        ev = coco_eval.COCOEvaluator(gt, tasks=(task,))
        for i, ds in by.items():
            ev.process(i, ds)
        wall, iou_ms, match_ms = [], [], []
        for it in range(a.warmup + a.iters):
            del spans[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ev.evaluate()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            iou_ms.append(sum(e0.elapsed_time(e1) for n, e0, e1 in spans if n != "umr_coco_match"))
            match_ms.append(sum(e0.elapsed_time(e1) for n, e0, e1 in spans if n == "umr_coco_match"))
        n = a.images
        rec[task] = {"device_ms_per_image": round(statistics.median(wall[a.warmup:]) / n, 4),
                     "kernels_ms_per_image": {"iou": round(statistics.median(iou_ms[a.warmup:]) / n, 4),
                                              "match": round(statistics.median(match_ms[a.warmup:]) / n, 4)},
                     "AP": out[task]["AP"], "AR100": out[task]["AR100"]}
        if task in host:
            rec[task]["host_ms_per_image"] = round(host[task], 2)
            rec[task]["host_over_device"] = round(host[task] / rec[task]["device_ms_per_image"], 1)
        if not a.no_host and a.images <= 16:
            want = Restatement(gt, dts, task).run()
            equal = equal and all((math.isnan(want[m]) and math.isnan(out[task][m])) or want[m] == out[task][m] for m in METRICS)
    if not a.no_host and a.images <= 16:
        rec["equal_to_restatement"] = equal
    rec["device_name"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    if not equal:
        raise SystemExit("the device evaluator and the restatement disagree")


if __name__ == "__main__":
    main()
