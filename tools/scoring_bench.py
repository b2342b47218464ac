"""Per-image time of object scoring (unmore_amd.object_scoring.Object_Scoring.score_image = the body of the reference's
main_object_scoring, object_scoring.py:182-255) and of what it takes to get the stage's `segmentation` strings, on the synthetic
640 x 480 six-object scene of tools/discovery_bench.py with a few hundred seeded boxes.

The networks are the stand-ins of tests/discovery_stubs.py (fields read back out of the crop) unless `--real-networks` is given
(ObjectnessNet dpt_large + Binary_Classifier, random weights, doing all their work; the stand-ins still supply the answers so that the
boxes surviving NMS are those of a scene with objects in it).  Four arms, the median of 20 after 3 warm-ups, stream-synchronised:
   (a) score_image                           what the class returned before it could encode: masks [K,H,W] on the device
   (b) (a) + masks.cpu()                     the copy any host-side encoder has to pay before it can start
   (c) score_image(segmentation=True, masks=False)   the strings from the fused kernel, no mask written
   (d) rle.encode(masks of (a))              the strings of masks that already are on the device, on its own
One JSON line per arm is appended to profiles/scoring_bench.jsonl.
python tools/scoring_bench.py [--real-networks] [--boxes 300]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from argparse import Namespace
from discovery_stubs import FieldsFromCrop, ObjectFraction
from unmore_amd import rle, synth
from unmore_amd.object_scoring import Object_Scoring

ap = argparse.ArgumentParser()
ap.add_argument("--real-networks", action="store_true")
ap.add_argument("--boxes", type=int, default=300)
opt = ap.parse_args()
dev = "cuda:0"
H, W = 480, 640
image = torch.from_numpy(synth.reasoning_scene(H, W, seed=2, n_objects=6)).to(dev)
rng = np.random.default_rng(0)
cx, cy = rng.uniform(0, W, opt.boxes), rng.uniform(0, H, opt.boxes)
bw, bh = rng.uniform(24, 320, opt.boxes), rng.uniform(24, 320, opt.boxes)
raw = np.stack([np.clip(cx - bw / 2, 0, W - 2), np.clip(cy - bh / 2, 0, H - 2), np.clip(cx + bw / 2, 2, W), np.clip(cy + bh / 2, 2, H)], 1)
raw = raw[(raw[:, 2] - raw[:, 0] >= 2) & (raw[:, 3] - raw[:, 1] >= 2)].tolist()

if opt.real_networks:
    from unmore_amd.binary_classifier import Binary_Classifier
    from unmore_amd.objectness_net import ObjectnessNet
    nargs = Namespace(use_bg_sdf=True, sdf_activation="tanh")
    torch.manual_seed(0)
    net = ObjectnessNet(dev, 128, "dpt_large", nargs).to(dev).eval()
    clf = Binary_Classifier(dev, 128, nargs).to(dev).eval()

    class Fields(torch.nn.Module):
        def get_prediction(self, images):
            net.get_prediction(images)
            return FieldsFromCrop()(images)
        forward = get_prediction

    class Existence(torch.nn.Module):
        def forward(self, images):
            clf(images)
            return ObjectFraction()(images)
    models = (Fields(), Existence())
else:
    models = (FieldsFromCrop(), ObjectFraction())
osc = Object_Scoring(Namespace(), dev, objectness_model=models[0], binary_classifier_model=models[1])

base = osc.score_image(image, raw)
masks = base["masks"]
strings = rle.encode(masks)
assert osc.score_image(image, raw, segmentation=True, masks=False)["segmentation"] == strings
arms = (("a: score_image", lambda: osc.score_image(image, raw)),
        ("b: score_image + masks.cpu()", lambda: osc.score_image(image, raw)["masks"].cpu()),
        ("c: score_image(segmentation=True, masks=False)", lambda: osc.score_image(image, raw, segmentation=True, masks=False)),
        ("d: rle.encode(masks)", lambda: rle.encode(masks)))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "scoring_bench.jsonl"), "a") as f:
    for name, fn in arms:
        times = []
        for i in range(23):
            torch.cuda.current_stream().synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            if i >= 3:
                times.append(time.perf_counter() - t0)
        row = {"arm": name, "networks": "real dpt_large" if opt.real_networks else "stand-ins", "image": [H, W], "boxes": len(raw), "K": len(masks),
               "mask_bytes": masks.numel(), "characters": sum(len(s["counts"]) for s in strings),
               "median_ms": round(statistics.median(times) * 1e3, 3), "min_ms": round(min(times) * 1e3, 3), "max_ms": round(max(times) * 1e3, 3),
               "runs": len(times), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(row), flush=True)
        f.write(json.dumps(row) + "\n")
