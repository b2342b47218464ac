"""The detector's input path on the device (unmore_amd.detector_input: map_batch + preprocess_image) beside the host path it replaces: one
JSON line per run, appended to profiles/detector_input_bench.jsonl.

    python tools/detector_input_bench.py --images 16 --iters 5 --warmup 2

The input is a seeded batch of `--images` 480x640 images with 20 elliptic blob masks each (decoded masks, bool), resized with the recipe's
INPUT.MIN_SIZE_TRAIN (240 ... 1024) / MAX_SIZE_TRAIN 1333 and flipped by draws made once.  Every time, the kernels' included, is the median
of `--iters` windows.
  device_ms:          map_batch + preprocess_image with the images and masks already on the device -- host checks and tables, one upload,
                      the launches, the one read of the keep flags -- as a host clock around both calls.
  device_upload_ms:   the same from pinned host tensors: the ORIGINAL images and mask stacks go up inside map_batch, one copy each.
  kernels_ms:         device events around each launch: resize (bilinear), masks (nearest + non-empty flags), normalise (+ pad + batch).
  bytes / floor_us:   the bytes each launch must move (inputs read once, outputs written once) and the time they take at the HBM rate
                      (8 TB/s, the MI355X's peak).
  resized_upload_ms:  the upload of the already resized batch alone (images uint8 [3,h,w], masks bool [20,h,w] from pinned memory):
                      what the host path would have to copy after its own resizes.
  host_ms:            the host path on `--procs` processes: PIL's resizes (Image.resize BILINEAR on RGB, NEAREST per mask) and the flips
                      if PIL is importable, else the numpy restatement of tests/det_input_common.py; `host_path` says which.  The
                      workers are fresh (spawned) processes that never open the GPU; they run and end before this process opens it.
`equal_to_restatement`: images, masks, boxes, sources and the normalised batch of EVERY image equal the numpy restatement's, and so do the
host arm's images and masks."""
import argparse
import json
import os
import statistics
import sys
import time
import multiprocessing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

H, W, N = 480, 640, 20
HBM_BYTES_PER_S = 8.0e12
PIXEL_MEAN, PIXEL_STD = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]


def make_image(seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    masks = np.zeros((N, H, W), dtype=bool)
    for k in range(N):
        cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(15, 120), rng.uniform(15, 160)
        masks[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return img, masks


def host_one(args):
    """one image through the host path: (image [3,h,w], masks [N,h,w])"""
    img, masks, (nh, nw, f), use_pil = args
    if use_pil:
        from PIL import Image
        out = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
        ms = np.stack([np.asarray(Image.fromarray(m.view(np.uint8)).resize((nw, nh), Image.NEAREST)) for m in masks])
    else:
        import det_input_common as C
        out, ms = C.resize_bilinear(img, nh, nw), C.resize_nearest(masks.view(np.uint8), nh, nw)
    if f == 1:
        out, ms = out[:, ::-1], ms[:, :, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1)), np.ascontiguousarray(ms).astype(bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detector_input_bench.jsonl"))
    args = ap.parse_args()
    from unmore_amd import detector_input as D
    import det_input_common as C
    try:
        import PIL  # noqa: F401
        use_pil = True
    except ImportError:
        use_pil = False

    B = args.images
    data = [make_image(args.seed * 1000 + i) for i in range(B)]
    transforms = D.draw_transforms([(H, W)] * B, min_size=D.MIN_SIZE_TRAIN, max_size=1333, np_random=np.random.RandomState(args.seed))
    boxes = []
    for _, masks in data:
        bs = []
        for m in masks:
            ys, xs = np.nonzero(m)
            bs.append([float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1)] if ys.size else [0.0, 0.0, 1.0, 1.0])
        boxes.append(bs)

    # the host arm first: fresh processes that never open the GPU, started and ended before this one opens it
    work = [(img, m, t, use_pil) for (img, m), t in zip(data, transforms)]
    t_host = []
    with multiprocessing.get_context("spawn").Pool(args.procs) as pool:
        pool.map(host_one, work[:args.procs], chunksize=1)           # the workers' imports are not timed
        for _ in range(args.iters):
            t0 = time.perf_counter()
            host_out = pool.map(host_one, work, chunksize=1)
            t_host.append((time.perf_counter() - t0) * 1e3)

    import torch
    assert torch.cuda.is_available(), "detector_input_bench needs the MI355X"
    pinned_img = [torch.from_numpy(img).pin_memory() for img, _ in data]
    pinned_msk = [torch.from_numpy(m).pin_memory() for _, m in data]

    def annotations(mask_tensors):
        return [[{"bbox": b, "bbox_mode": D.XYXY_ABS, "segmentation": m[j]} for j, b in enumerate(bs)] for m, bs in zip(mask_tensors, boxes)]

    dev_img = [t.cuda() for t in pinned_img]
    dev_ann = annotations([t.cuda() for t in pinned_msk])
    host_ann = annotations(pinned_msk)

    def run(images, ann, phases=None):
        items = D.map_batch(images, ann, transforms, _phase_ms=phases)
        batch, sizes = D.preprocess_image(items, PIXEL_MEAN, PIXEL_STD, 32, _phase_ms=phases)
        return items, batch

    t_dev, t_up, t_resized, phases = [], [], [], []
    items = batch = None
    for i in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        items, batch = run(dev_img, dev_ann)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out2 = run(pinned_img, host_ann)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del out2
        if i >= args.warmup:
            t_dev.append((t1 - t0) * 1e3)
            t_up.append((t2 - t1) * 1e3)
            phases.append({})
            run(dev_img, dev_ann, phases[-1])
    kernels = {k: round(statistics.median(p[k] for p in phases), 4) for k in phases[0]}

    # the upload the host path would make: the resized batch
    res_img = [torch.empty((3, nh, nw), dtype=torch.uint8).pin_memory() for nh, nw, _ in transforms]
    res_msk = [torch.empty((N, nh, nw), dtype=torch.bool).pin_memory() for nh, nw, _ in transforms]
    for i in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        up = [t.to("cuda", non_blocking=True) for t in res_img + res_msk]
        torch.cuda.synchronize()
        if i >= args.warmup:
            t_resized.append((time.perf_counter() - t0) * 1e3)
        del up

    # bytes each launch must move
    out_px = [nh * nw for nh, nw, _ in transforms]
    Hp = -(-max(t[0] for t in transforms) // 32) * 32
    Wp = -(-max(t[1] for t in transforms) // 32) * 32
    moved = {"resize": sum(3 * H * W + 3 * p for p in out_px), "masks": sum(N * H * W + N * p for p in out_px),
             "normalise": sum(3 * p for p in out_px) + B * 3 * Hp * Wp * 4}
    floor_us = {k: round(v / HBM_BYTES_PER_S * 1e6, 2) for k, v in moved.items()}

    equal = True
    for k in range(B):
        img, masks = data[k]
        ref = C.map_reference(img, [{"bbox": b, "bbox_mode": C.XYXY_ABS, "segmentation": m} for b, m in zip(boxes[k], masks)], transforms[k])
        equal &= np.array_equal(items[k]["image"].cpu().numpy(), ref["image"]) and np.array_equal(items[k]["masks"].cpu().numpy(), ref["masks"])
        equal &= np.array_equal(items[k]["boxes"].cpu().numpy(), ref["boxes"]) and np.array_equal(items[k]["source"].cpu().numpy(), ref["source"])
        equal &= np.array_equal(host_out[k][0], ref["image"]) and np.array_equal(host_out[k][1][ref["keep"]], ref["masks"])
        want = ((ref["image"].astype(np.float32) - np.float32(PIXEL_MEAN).reshape(3, 1, 1)) / np.float32(PIXEL_STD).reshape(3, 1, 1))
        got = batch[k, :, :transforms[k][0], :transforms[k][1]].cpu().numpy()
        equal &= np.array_equal(got.view(np.uint32), want.view(np.uint32))
    med = statistics.median
    line = {"tool": "detector_input_bench", "images": B, "hw": [H, W], "masks_per_image": N, "iters": args.iters, "warmup": args.warmup,
            "shapes": [list(t) for t in transforms], "batch": list(batch.shape), "instances_out": [int(it["masks"].shape[0]) for it in items],
            "device_ms": round(med(t_dev), 3), "device_upload_ms": round(med(t_up), 3), "kernels_ms": kernels, "bytes": moved,
            "floor_us": floor_us, "resized_upload_ms": round(med(t_resized), 3), "host_path": "PIL" if use_pil else "numpy restatement",
            "host_procs": args.procs, "host_ms": round(med(t_host), 1), "equal_to_restatement": bool(equal),
            "host_over_device_upload": round(med(t_host) / med(t_up), 1), "device_name": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
