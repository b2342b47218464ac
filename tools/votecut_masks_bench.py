"""Training masks from VoteCut annotations (VoteCutAnnotations.masks: run-length strings -> top-1 largest-component mask + union mask on
the device) against the host path they replace: one JSON line per run, appended to profiles/votecut_masks_bench.jsonl.

    python tools/votecut_masks_bench.py --batch 20  --iters 20 --warmup 3
    python tools/votecut_masks_bench.py --batch 256 --iters 5  --warmup 2

Every image is 375x500 with `--anns` annotations of smoothed-noise blobs (30 % set, a few components); a "mask" below is one image's pair
(top-1 single-component mask, full mask), so masks_per_s counts images.  Three arms, each timed as a host clock around work that ends in
a device synchronise, `--repeats` windows of `--iters` calls; the median window is reported with the fastest and the slowest:
  host:   rle.decode_numpy + scipy.ndimage.label + np.bincount for the top-1 mask, decode_numpy + OR for the full mask, in this one
          process, then the upload of both masks.  It stands in for pycocotools + cv2, which are not installed where this was written;
          their C loops are faster than numpy's, so this is the host path as this project can run it, not OpenCV's speed.
  upload: the two ready-made masks per image copied to the device, nothing else: the floor of any path that makes masks on the host.
  device: VoteCutAnnotations.masks -- per call two packed uploads (tables + characters), four launches, two status read-backs.
device_split_ms: the same call's two halves timed with device events (mode 1 = parse + largest component over the top-1 records,
mode 0 = parse + union paint over all records).
kernels: the split by kernel, from a kernel trace of a second run of this tool (a fresh child process under
`rocprofv3 --kernel-trace --stats`, device arm only, started after the untraced windows are over): per kernel the launches, the mean
time per launch and the time per VoteCutAnnotations.masks call (rle_parse_kernel runs twice per call, once per mode).
--no-kernel-trace skips it."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 375, 500


KERNELS = ("rle_parse_kernel", "rle_largest_kernel", "rle_union_paint_kernel")


def blob(seed):
    """a smoothed-noise blob mask of 0/1: a few components, a few hundred runs, 30 % set"""
    from scipy import ndimage
    f = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((H, W)), sigma=min(H, W) / 12.0)
    return (f > np.quantile(f, 0.7)).astype(np.uint8)


def kernel_split(a):
    """the device arm again in a child process under rocprofv3; the rows of its kernel_stats.csv that belong to csrc/rle_decode.hip"""
    with tempfile.TemporaryDirectory() as tmp:
        child_out = os.path.join(tmp, "child.jsonl")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(tmp, "trace"), "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--device-only", "--no-kernel-trace", "--batch", str(a.batch), "--anns", str(a.anns),
               "--iters", str(a.iters), "--warmup", str(a.warmup), "--repeats", "1", "--out", child_out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("the traced run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        with open(child_out) as f:
            calls = json.loads(f.readline())["masks_calls"]
        files = glob.glob(os.path.join(tmp, "trace", "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("the traced run wrote no kernel_stats.csv")
        out = {}
        with open(files[0], newline="") as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if k in row["Name"]:
                        out[k] = {"launches": int(row["Calls"]), "us_per_launch": round(float(row["AverageNs"]) / 1e3, 2),
                                  "us_per_masks_call": round(float(row["TotalDurationNs"]) / 1e3 / calls, 2)}
        if set(out) != set(KERNELS):
            raise RuntimeError(f"kernel_stats.csv lacks some of {KERNELS}: found {sorted(out)}")
        return out


def make_annotations(B, n_anns, distinct=32):
    from unmore_amd import rle
    rng = np.random.default_rng(0)
    base = [[rle.encode_numpy(blob(100 * k + j)) for j in range(n_anns)] for k in range(min(B, distinct))]
    images, anns = [], []
    for i in range(B):
        images.append({"id": i, "file_name": f"n{i // 100:04d}/im{i}.JPEG", "height": H, "width": W})
        for j, seg in enumerate(base[i % len(base)]):
            anns.append({"id": i * n_anns + j, "image_id": i, "weight": float(rng.random()), "segmentation": seg})
    return {"images": images, "annotations": anns}


def host_masks(ann, ids):
    from scipy import ndimage
    from unmore_amd import rle
    top1, full = [], []
    for i in ids:
        m = rle.decode_numpy(ann.top1(i)["segmentation"])
        lab, n = ndimage.label(m)
        if n:
            m = lab == 1 + int(np.argmax(np.bincount(lab.reshape(-1))[1:]))
        top1.append(np.ascontiguousarray(m, dtype=np.uint8) * 255)
        u = np.zeros((H, W), np.uint8)
        for r in ann.records(i):
            u |= rle.decode_numpy(r)
        full.append(u * 255)
    return top1, full


def windows(fn, iters, warmup, repeats):
    """ms per call: (median, fastest, slowest) over `repeats` windows of `iters` calls, each ending in a synchronise"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--anns", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=1, help="calls per window of the host arm (it is slow)")
    ap.add_argument("--device-only", action="store_true", help="the device arm alone (what the kernel trace runs)")
    ap.add_argument("--no-kernel-trace", action="store_true", help="skip the traced child run that gives the split by kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "votecut_masks_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("votecut_masks_bench measures on the MI355X; no GPU found")
    from unmore_amd import VoteCutAnnotations, rle
    B = a.batch
    dev = torch.device("cuda:0")
    d = make_annotations(B, a.anns)
    ann = VoteCutAnnotations(d)
    ids = ann.image_ids
    nchars = [len(x["segmentation"]["counts"]) for x in d["annotations"]]
    rec = {"tool": "votecut_masks_bench", "batch": B, "annotations_per_image": a.anns, "hw": [H, W], "iters": a.iters, "warmup": a.warmup,
           "repeats": a.repeats, "chars_per_string_mean": round(float(np.mean(nchars)), 1), "chars_per_string_max": int(max(nchars))}

    def stat(name, m, per_s=True):
        med, lo, hi = m
        rec[name + "_ms"] = round(med, 3)
        rec[name + "_ms_min_max"] = [round(lo, 3), round(hi, 3)]
        if per_s:
            rec[name + "_masks_per_s"] = round(B / med * 1e3, 1)

    h_top1, h_full = host_masks(ann, ids)
    # the device path gives the host's bytes at the sizes timed
    top1, full = ann.masks(ids, device=dev)
    assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(top1, h_top1)) and all(np.array_equal(f.cpu().numpy(), h) for f, h in zip(full, h_full))
    rec["equal_to_host"] = True

    stat("device", windows(lambda: ann.masks(ids, device=dev), a.iters, a.warmup, a.repeats))
    top1_records = [ann.top1(i)["segmentation"] for i in ids]
    all_records = [r for i in ids for r in ann.records(i)]
    groups = [(len(ann.records(i)), (H, W)) for i in ids]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    split = []
    for _ in range(a.warmup + a.iters):
        ev[0].record()
        rle.largest_component(top1_records, device=dev)
        ev[1].record()
        rle.decode(all_records, groups=groups, device=dev)
        ev[2].record()
        torch.cuda.synchronize()
        split.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    split = split[a.warmup:]
    rec["device_split_ms"] = {"largest_component_call": round(statistics.median(s[0] for s in split), 3),
                              "union_decode_call": round(statistics.median(s[1] for s in split), 3)}
    if not a.device_only:
        def upload():
            return [torch.from_numpy(m).to(dev) for m in h_top1], [torch.from_numpy(m).to(dev) for m in h_full]

        def host():
            t, f = host_masks(ann, ids)
            return [torch.from_numpy(m).to(dev) for m in t], [torch.from_numpy(m).to(dev) for m in f]
        stat("upload", windows(upload, a.iters, a.warmup, a.repeats))
        stat("host", windows(host, a.host_iters, 1, min(a.repeats, 3)))
        rec["speedup_over_host"] = round(rec["host_ms"] / rec["device_ms"], 2)
        rec["speedup_over_upload"] = round(rec["upload_ms"] / rec["device_ms"], 2)
    rec["masks_calls"] = 1 + a.warmup + a.iters * a.repeats + len(split) + a.warmup      # launches of each mode in this process
    failed = None
    if not a.no_kernel_trace:
        try:
            rec["kernels"] = kernel_split(a)
        except (RuntimeError, OSError, subprocess.TimeoutExpired, KeyError, ValueError) as e:      # the timed arms above are still worth their line
            rec["kernels"], failed = None, str(e)
    rec["device_name"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    if failed:
        raise SystemExit("no split by kernel: " + failed)


if __name__ == "__main__":
    main()
