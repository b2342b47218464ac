"""unmore_amd.coco_eval without a GPU: the plain restatement the GPU tests compare against (tests/coco_eval_common.py) pinned on cases
worked out by hand, the host half of the evaluator (accumulate / summarize) against that restatement, the new exports, and the
argument errors that are raised before any launch."""
import math
import os
import re

import numpy as np
import pytest

from unmore_amd import _lib, coco_eval, rle
from coco_eval_common import (AREA_RNG, IOU_THRS, METRICS, Restatement, box_iou_numpy, dataset, dt_ann, evaluate_img, gt_ann, mask_iou_numpy,
                              rect, seeded_scene)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("umr_mask_iou_workspace", "umr_mask_iou", "umr_box_iou", "umr_coco_match")


def _near(x, v):
    return abs(x - v) <= 1e-9            # precision is tp / (tp + fp + spacing(1)): 1 - 2e-16 where it "is" 1


def test_every_ground_truth_detected_perfectly():
    """one ground truth per image (so AR1 can reach 1), a small one and a medium one, none large"""
    small, medium = rect(80, 100, 3, 4, 10, 20), rect(80, 100, 10, 10, 50, 60)          # areas 200 and 3000
    gt = dataset([(1, 80, 100), (2, 80, 100)], [gt_ann(1, 1, small), gt_ann(2, 2, medium)])
    dts = [dt_ann(1, small, 0.9), dt_ann(2, medium, 0.8)]
    for task in ("segm", "bbox"):
        res = Restatement(gt, dts, task).run()
        for name in METRICS:
            if name in ("APl", "ARl"):
                assert math.isnan(res[name]), (task, name)
            else:
                assert _near(res[name], 100.0), (task, name, res[name])


def test_two_ground_truths_one_perfect_detection():
    a, b = rect(40, 40, 2, 2, 10, 10), rect(40, 40, 20, 20, 10, 10)
    gt = dataset([(1, 40, 40)], [gt_ann(1, 1, a), gt_ann(2, 1, b)])
    r = Restatement(gt, [dt_ann(1, a, 0.5)], "segm")
    res = r.run()
    assert _near(res["AP"], 100.0 * 51 / 101) and _near(res["AR100"], 50.0) and _near(res["AR1"], 50.0)     # 51 recall points 0.00 .. 0.50
    p = r.eval["precision"][0, :, 0, 0, 2]
    assert (p[:51] > 0.999999).all() and (p[51:] == 0).all()
    assert r.eval["scores"][0, 50, 0, 0, 2] == 0.5 and r.eval["scores"][0, 51, 0, 0, 2] == 0
    assert (r.eval["precision"][:, :, 0, 3, :] == -1).all()             # no large ground truth: undefined, not zero


def test_iou_of_exactly_one_half_matches_at_the_first_threshold_only():
    g = np.zeros((5, 5), np.uint8)
    g[1, 1] = g[2, 1] = 1
    d = np.zeros((5, 5), np.uint8)
    d[1, 1] = 1
    iou = mask_iou_numpy([rle.encode_numpy(d)], [rle.encode_numpy(g)], [0])
    assert iou[0, 0] == 0.5
    e = evaluate_img(iou, [1.0], [1], [2], [0], AREA_RNG[0], IOU_THRS, 100)
    assert e["dtm"][:, 0].tolist() == [True] + [False] * 9 and e["dtg"][:, 0].tolist() == [0] + [-1] * 9
    assert iou[0, 0] >= IOU_THRS[0] and not iou[0, 0] >= IOU_THRS[1]


def test_a_detection_matched_to_a_crowd_is_ignored():
    obj, crowd = rect(60, 60, 2, 2, 12, 12), rect(60, 60, 30, 5, 25, 50)
    inside = rect(60, 60, 32, 10, 10, 10)                                    # wholly inside the crowd region: i / a_d = 1
    gt = dataset([(1, 60, 60)], [gt_ann(1, 1, obj), gt_ann(2, 1, crowd, iscrowd=1)])
    dts = [dt_ann(1, inside, 0.9), dt_ann(1, obj, 0.8)]                      # the crowd's detection scores higher
    r = Restatement(gt, dts, "segm")
    res = r.run()
    assert _near(res["AP"], 100.0) and _near(res["AR100"], 100.0)            # as a false positive it would halve the precision
    e = r.eval_imgs[1, 0, 1]
    assert e["dtm"][:, 0].all() and e["dtIg"][:, 0].all() and (e["dtg"][:, 0] == 1).all()
    assert e["dtm"][:, 1].all() and not e["dtIg"][:, 1].any()
    assert mask_iou_numpy([rle.encode_numpy(inside)], [rle.encode_numpy(crowd)], [1])[0, 0] == 1.0
    # the same detection against a non-crowd copy: a plain false positive
    gt2 = dataset([(1, 60, 60)], [gt_ann(1, 1, obj), gt_ann(2, 1, crowd)])
    assert Restatement(gt2, dts, "segm").run()["AP"] < 60


def test_walk_order_ties_and_area_bounds_by_hand():
    # two identical ground truths, IoU tie: the LATER one is taken first, the earlier by the next detection
    iou = np.array([[0.8, 0.8], [0.8, 0.8], [0.8, 0.8]])
    e = evaluate_img(iou, [3, 2, 1], [100, 100, 100], [100, 100], [0, 0], AREA_RNG[0], IOU_THRS, 100)
    assert e["dtg"][0].tolist() == [1, 0, -1] and e["dtg"][7].tolist() == [-1, -1, -1]           # 0.8 < 0.85
    # areas exactly 1024 and 9216 are inside both neighbouring ranges
    for a, want in ((1, [False, True]), (2, [False, False]), (3, [True, False])):
        e = evaluate_img(np.zeros((0, 2)), [], [], [1024, 9216], [0, 0], AREA_RNG[a], IOU_THRS, 100)
        assert e["gtIg"].tolist() == want
    # the best ground truth is taken: fall through to the ignored one, and inherit its flag
    iou = np.array([[0.9, 0.6], [0.7, 0.6]])
    e = evaluate_img(iou, [2, 1], [50, 50], [50, 5000], [0, 0], AREA_RNG[1], IOU_THRS, 100)
    assert e["dtg"][0].tolist() == [0, 1] and e["dtIg"][0].tolist() == [False, True]
    # bbIou: touching boxes do not overlap, a nested box gives the area ratio
    b = box_iou_numpy([[0, 0, 10, 10], [2, 2, 4, 4]], [[10, 0, 5, 5], [0, 0, 10, 10]], [0, 0])
    assert b.tolist() == [[0.0, 1.0], [0.0, 0.16]]


def test_host_accumulate_and_summarize_equal_the_restatement():
    gt, dts = seeded_scene(5, n_images=3, H=48, W=64, n_gt=4, n_noise=3)
    r = Restatement(gt, dts, "segm", max_dets=(1, 3, 5))
    want = r.run()
    per_unit, scores = [], []
    for img in r.img_ids:
        es = [r.eval_imgs[1, a, img] for a in range(4)]
        per_unit.append(None if es[0] is None else {"dtm": np.stack([e["dtm"] for e in es]), "dtig": np.stack([e["dtIg"] for e in es]),
                                                    "gtig": np.stack([e["gtIg"] for e in es])})
        scores.append([] if es[0] is None else es[0]["scores"])
    ev = coco_eval.accumulate(per_unit, scores, [0] * len(per_unit), 1, [1, 3, 5])
    for k in ("precision", "recall", "scores"):
        assert ev[k].dtype == np.float64 and ev[k].tobytes() == r.eval[k].tobytes(), k
    stats = coco_eval.summarize(ev, [1, 3, 5])
    assert stats.tobytes() == r.stats.tobytes()
    assert (coco_eval.IOU_THRS == IOU_THRS).all() and coco_eval.IOU_THRS[5] == 0.75 and tuple(coco_eval.METRICS) == tuple(METRICS)
    assert want["AP"] == stats[0] * 100


def test_exports_are_declared_and_resolvable():
    with open(os.path.join(ROOT, "include", "umr.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None
    ws = lib.umr_mask_iou_workspace
    assert ws(-1, 0, 0) == -1 and ws(1, -1, 0) == -1 and ws(1, 0, -1) == -1
    # nruns + numbers + starts + extents + the bit words
    assert ws(3, 10, 100) >= 3 * 4 + 13 * 12 + 3 * 8 + 100 * 8
    assert ws(3, 10, 101) - ws(3, 10, 100) == 8
    # argument checks answer before any launch
    assert lib.umr_mask_iou(None, None, 0, 0, None, None, None, None, None, None, 0, 1, 0, 0, 0, 0, None, None, None, None, None, 0, None) == -1
    assert b"mask_iou" in lib.umr_last_error_string()
    assert lib.umr_box_iou(None, None, None, None, None, 1, 0, 0, 0, None, None) == -1
    assert lib.umr_coco_match(None, None, 0, None, None, None, 0, None, 0, None, None, None, None, 0, None, 10, 100, 1, None, None, None, None,
                              None, None) == -1
    assert b"coco_match" in lib.umr_last_error_string()


def test_argument_errors_are_raised_before_any_launch():
    """device='cpu' would raise RuntimeError at the first launch: every one of these is a ValueError, so none got that far"""
    m = rect(12, 12, 2, 2, 4, 4)
    gt = dataset([(1, 12, 12)], [gt_ann(1, 1, m)])
    polygon = dataset([(1, 12, 12)], [dict(gt_ann(7, 1, m), segmentation=[[2.0, 2.0, 6.0, 2.0, 6.0, 6.0]])])

    def run(g, dts, tasks=("bbox", "segm")):
        ev = coco_eval.COCOEvaluator(g, tasks=tasks, device="cpu")
        for d in dts:
            ev.process(d["image_id"], [d])
        return ev.evaluate()
    with pytest.raises(ValueError, match="annotation 7.*polygon"):
        run(polygon, [dt_ann(1, m, 0.5)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # bbox reads no segmentation: it gets as far as the launch
        run(polygon, [dt_ann(1, m, 0.5)], tasks=("bbox",))
    with pytest.raises(ValueError, match="image 5"):
        run(gt, [dt_ann(5, m, 0.5)])
    with pytest.raises(ValueError, match="mixed mask sizes"):
        run(gt, [dt_ann(1, rect(12, 13, 2, 2, 4, 4), 0.5)])
    with pytest.raises(ValueError, match="mixed mask sizes"):
        coco_eval.mask_iou([rle.encode_numpy(m)], [rle.encode_numpy(rect(13, 12, 1, 1, 2, 2))], [0], device="cpu")
    with pytest.raises(ValueError, match="polygon"):
        coco_eval.mask_iou([[[1.0, 1.0, 4.0, 1.0, 4.0, 4.0]]], [rle.encode_numpy(m)], [0], device="cpu")
    with pytest.raises(ValueError, match="iscrowd"):
        coco_eval.mask_iou([rle.encode_numpy(m)], [rle.encode_numpy(m)], [0, 0], device="cpu")
    with pytest.raises(ValueError, match=r"\[x, y, w, h\]"):
        coco_eval.box_iou([[0, 0, 1]], [[0, 0, 1, 1]], [0], device="cpu")
    with pytest.raises(ValueError, match="unknown task"):
        coco_eval.COCOEvaluator(gt, tasks=("keypoints",))
    for call in (lambda: coco_eval.mask_iou([rle.encode_numpy(m)], [rle.encode_numpy(m)], [0], device="cpu"),
                 lambda: coco_eval.box_iou([[0, 0, 1, 1]], [[0, 0, 1, 1]], [0], device="cpu"),
                 lambda: run(gt, [dt_ann(1, m, 0.5)])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert coco_eval.COCOEvaluator(gt, device="cpu").evaluate() == {}       # nothing processed: nothing to evaluate, as the reference
    assert coco_eval.COCOEvaluator(gt, max_dets_per_image=300).max_dets == [1, 10, 300]


def test_evaluate_ap_defaults(tmp_path):
    """main.py:24-70: grouping by image, score from weight or 1, id from the position; the evaluator is a stub here"""
    import json

    class Stub:
        def reset(self):
            self.seen = []

        def process(self, image_id, coco_instances):
            self.seen.append((image_id, coco_instances))

        def evaluate(self):
            return {"bbox": {"AP": 1.0}}
    preds = [{"image_id": 3, "weight": 0.25}, {"image_id": 1, "score": 0.5, "id": 40}, {"image_id": 3}]
    (tmp_path / "p.json").write_text(json.dumps(preds))
    stub = Stub()
    out = coco_eval.evaluate_ap("gt.json", str(tmp_path / "p.json"), stub, str(tmp_path / "res"))
    assert [i for i, _ in stub.seen] == [3, 1]
    assert [(a["id"], a["score"]) for a in stub.seen[0][1]] == [(0, 0.25), (2, 1)] and stub.seen[1][1][0]["id"] == 40
    written = json.loads((tmp_path / "res" / "ap_score.json").read_text())
    assert written == out and written["number_of_images"] == 2 and written["number_of_annotations"] == 3
    assert written["gt_annotation_path"] == "gt.json" and written["pred_annotation_path"].endswith("p.json") and written["bbox"] == {"AP": 1.0}
