"""unmore_amd.coco_eval on the device against the plain numpy restatement (tests/coco_eval_common.py).  Every comparison is exact: integer
intersections and areas, IoU matrices bit for bit as float64, match / ignore tables, the precision / recall / scores arrays bit for bit,
the twelve statistics.  Nothing here is approximate, so there is no tolerance."""
import json
import math

import numpy as np
import pytest
import torch

from unmore_amd import coco_eval, rle
from coco_eval_common import (AREA_RNG, IOU_THRS, METRICS, Restatement, blob, box_iou_numpy, dataset, dt_ann, evaluate_img, gt_ann,
                              mask_counts_numpy, mask_iou_numpy, rect, seeded_scene)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _mask_set(H, W, seed):
    """the word-boundary cases of one size: empty, full, the four corners, a run over several columns, halves, random"""
    rng = np.random.default_rng(seed)
    out = [np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)]
    for y, x in ((0, 0), (H - 1, 0), (0, W - 1), (H - 1, W - 1)):
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 1
        out.append(m)
    cols = np.zeros((H, W), np.uint8)
    cols[:, 3:7] = 1                                      # four whole columns: ONE run of 4*H pixels
    cols[H // 2:, 2] = 1                                  # ... that starts in the middle of the column before
    out.append(cols)
    out.append(rect(H, W, 0, 0, H, W // 2))
    out.append((rng.random((H, W)) < 0.5).astype(np.uint8))
    out.append((rng.random((H, W)) < 0.05).astype(np.uint8))
    out.append(blob(H, W, H / 2, W / 2, H / 3, W / 4))
    return out


def _check_mask_unit(got, dt, gt, crowd):
    inter, da, ga = mask_counts_numpy(dt, gt)
    assert got["inter"].dtype == torch.int32 and got["iou"].dtype == torch.float64
    assert (got["inter"].cpu().numpy() == inter).all()
    assert (got["dt_area"].cpu().numpy() == da).all() and (got["gt_area"].cpu().numpy() == ga).all()
    assert _bits(got["iou"].cpu().numpy()) == _bits(mask_iou_numpy(dt, gt, crowd))


def test_mask_iou_word_boundaries_three_sizes_in_one_call():
    units = []
    for s, (H, W) in enumerate(((37, 53), (64, 64), (70, 129))):      # column heights below, at and above a 64-bit word
        ms = [rle.encode_numpy(m) for m in _mask_set(H, W, s)]
        units.append((ms, ms[::-1], [int(i % 4 == 1) for i in range(len(ms))]))
    got = coco_eval.mask_iou_units(units)
    for g, (dt, gt, crowd) in zip(got, units):
        _check_mask_unit(g, dt, gt, crowd)
    again = coco_eval.mask_iou_units(units)
    for a, b in zip(got, again):
        assert torch.equal(a["inter"], b["inter"]) and a["iou"].cpu().numpy().tobytes() == b["iou"].cpu().numpy().tobytes()
    one = coco_eval.mask_iou(units[0][0], units[0][1], units[0][2])
    assert one.shape == (11, 11) and one.is_cuda and torch.equal(one, got[0]["iou"])


def test_mask_iou_unit_shapes():
    rng = np.random.default_rng(11)
    H, W = 40, 70
    many = [rle.encode_numpy(blob(H, W, rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, 15), rng.uniform(1, 25))) for _ in range(130)]
    gts = [rle.encode_numpy(blob(H, W, rng.uniform(0, H), rng.uniform(0, W), rng.uniform(3, 15), rng.uniform(3, 25))) for _ in range(11)]
    small = [rle.encode_numpy(m) for m in _mask_set(9, 5, 3)]
    counts = {"size": [9, 5], "counts": [int(c) for c in rle.mask_to_counts(_mask_set(9, 5, 3)[8])]}      # an uncompressed record
    units = [([], gts[:2], [0, 0]), (small[:3], [], []), ([], [], []), (many, gts, [0] * 10 + [1]), (small + [counts], small[:2], [0, 1])]
    got = coco_eval.mask_iou_units(units)
    assert [tuple(g["iou"].shape) for g in got] == [(0, 2), (3, 0), (0, 0), (130, 11), (12, 2)]
    for g, (dt, gt, crowd) in zip(got, units):
        _check_mask_unit(g, dt, gt, crowd)
    assert coco_eval.mask_iou_units([]) == []
    assert coco_eval.mask_iou([], [], []).shape == (0, 0)


def test_mask_iou_one_malformed_string_among_good_ones():
    H, W = 33, 21
    ms = [rle.encode_numpy(m) for m in _mask_set(H, W, 4)]
    bad = dict(ms[8], counts=ms[8]["counts"][:-2])                      # counts that no longer sum to H*W
    dt, gt, crowd = ms[:4] + [bad] + ms[4:], ms[6:], [0, 1, 0, 0, 0]
    with pytest.raises(ValueError, match="record 8") as ei:           # records count on through the call: 4 of the first unit, then 4 good ones
        coco_eval.mask_iou_units([(ms[:2], ms[:2], [0, 0]), (dt, gt, crowd)])
    st = ei.value.status
    assert st.shape == (4 + 12 + 5,) and st[4 + 4] != 0 and (np.delete(st, 8) == 0).all()
    empty = rle.encode_numpy(np.zeros((H, W), np.uint8))               # a malformed record contributes nothing
    _check_mask_unit(ei.value.units[0], ms[:2], ms[:2], [0, 0])
    _check_mask_unit(ei.value.units[1], ms[:4] + [empty] + ms[4:], gt, crowd)


def test_box_iou_is_not_contracted():
    rng = np.random.default_rng(21)
    dt = (rng.random((70, 4)) * 100).tolist()                          # non-dyadic: w*h is inexact, so a fused da + ga - w*h would differ
    gt = (rng.random((9, 4)) * 100).tolist()
    dt += [[gt[0][0] + gt[0][2], gt[0][1], 7.3, 5.1],                  # touches ground truth 0 on its right edge
           [gt[1][0] + gt[1][2] / 3, gt[1][1] + gt[1][3] / 3, gt[1][2] / 3, gt[1][3] / 3],        # nested inside ground truth 1
           list(gt[2]), [0.1, 0.2, 0.0, 0.0]]                          # identical; degenerate
    crowd = [0, 0, 0, 1, 0, 1, 0, 0, 0]
    want = box_iou_numpy(dt, gt, crowd)
    got = coco_eval.box_iou(dt, gt, crowd)
    assert got.dtype == torch.float64 and got.is_cuda and _bits(got.cpu().numpy()) == _bits(want)
    assert want[70, 0] == 0.0 and abs(want[71, 1] - 1 / 9) < 1e-12 and abs(want[72, 2] - 1) < 1e-12      # what the special boxes are there for
    units = [(dt[:3], [], []), ([], gt, crowd), (dt, gt, crowd), ([], [], []), (gt, gt[::-1], crowd)]
    for g, (d, q, c) in zip(coco_eval.box_iou_units(units), units):
        assert _bits(g.cpu().numpy()) == _bits(box_iou_numpy(d, q, c)) and tuple(g.shape) == (len(d), len(q))


def _match_cases():
    rng = np.random.default_rng(31)
    cases = []
    # duplicate ground truths and duplicate detections: IoU ties go to the later ground truth
    cases.append((np.array([[0.8, 0.8, 0.3], [0.8, 0.8, 0.3], [0.8, 0.8, 0.6], [0.5, 0.5, 0.5]]), [500] * 4, [500, 500, 500], [0, 0, 0]))
    # the best ground truth is already taken: fall through to an ignored one (area out of "small"), then to nothing
    cases.append((np.array([[0.9, 0.6, 0.0], [0.7, 0.6, 0.0], [0.7, 0.65, 0.0]]), [50, 50, 50], [50, 5000, 20000], [0, 0, 0]))
    # one crowd matched by three detections; a plain ground truth after it
    cases.append((np.array([[1.0, 0.0], [1.0, 0.1], [0.9, 0.0], [0.2, 0.95]]), [100, 200, 300, 400], [4000, 400], [1, 0]))
    # areas exactly on the bounds; unmatched detections inside and outside the ranges
    cases.append((np.array([[0.0, 0.0, 0.7], [0.0, 0.0, 0.0], [0.6, 0.0, 0.0], [0.0, 0.0, 0.0]]), [1024, 9216, 1023.5, 9216.5],
                  [1024, 9216, 1025], [0, 0, 0]))
    # 130 detections against maxDet 100, quantised IoUs
    cases.append((np.round(rng.random((130, 7)), 1), rng.uniform(10, 20000, 130), rng.uniform(10, 20000, 7), [0, 0, 1, 0, 0, 0, 1]))
    # more ground truths than a wave has lanes, heavy ties
    cases.append((np.round(rng.random((40, 150)), 1), rng.uniform(10, 20000, 40), rng.uniform(10, 20000, 150), (rng.random(150) < 0.1).astype(int)))
    cases.append((np.zeros((0, 3)), [], [10, 2000, 30000], [0, 1, 0]))          # ground truths, no detection
    cases.append((np.zeros((3, 0)), [10, 2000, 30000], [], []))                 # detections, no ground truth
    cases.append((np.zeros((0, 0)), [], [], []))
    cases.append((np.round(rng.random((64, 64)), 2), rng.uniform(10, 20000, 64), rng.uniform(10, 20000, 64), [0] * 64))
    return cases


def test_matching_equals_the_sequential_walk():
    cases = _match_cases()
    got = coco_eval.match_units([(torch.from_numpy(np.ascontiguousarray(i, dtype=np.float64)).cuda(), da, ga, gc) for i, da, ga, gc in cases],
                                max_det=100)
    assert len(got) == len(cases)
    for n, (g, (iou, da, ga, gc)) in enumerate(zip(got, cases)):
        D, G = iou.shape
        assert g["dtm"].shape == (4, 10, D) and g["gtig"].shape == (4, G) and g["gtm"].shape == (4, 10, G)
        for a in range(4):
            e = evaluate_img(iou, np.zeros(D), da, ga, gc, AREA_RNG[a], IOU_THRS, 100)
            De = min(D, 100)
            assert (g["dtm"][a][:, :De] == e["dtm"]).all(), (n, a)
            assert (g["dtg"][a][:, :De] == e["dtg"]).all(), (n, a)
            assert (g["dtig"][a][:, :De] == e["dtIg"]).all(), (n, a)
            assert (g["gtig"][a] == e["gtIg"]).all() and (g["gtm"][a] == e["gtm"]).all(), (n, a)
            assert not g["dtm"][a][:, De:].any() and (g["dtg"][a][:, De:] == -1).all() and g["dtig"][a][:, De:].all()
    # the hand-worked outcomes, so the comparison above is not two copies of one mistake
    assert got[0]["dtg"][0, 0].tolist() == [1, 0, 2, -1]
    assert got[1]["dtg"][1, 0].tolist() == [0, 1, -1] and got[1]["dtig"][1, 0].tolist() == [False, True, False]
    assert got[2]["dtg"][0, 0].tolist() == [0, 0, 0, 1] and got[2]["dtig"][0, 0].tolist() == [True, True, True, False]
    assert got[3]["gtig"].tolist() == [[False] * 3, [False, True, True], [False, False, False], [True, False, True]]
    assert got[3]["dtig"][1, 0].tolist() == [True, True, False, True] and got[3]["dtig"][2, 0].tolist() == [False, False, False, True]
    # a smaller maxDet through the same kernel
    small = coco_eval.match_units([(torch.from_numpy(cases[4][0]).cuda(), cases[4][1], cases[4][2], cases[4][3])], max_det=10)[0]
    e = evaluate_img(cases[4][0], np.zeros(130), cases[4][1], cases[4][2], cases[4][3], AREA_RNG[0], IOU_THRS, 10)
    assert (small["dtg"][0][:, :10] == e["dtg"]).all() and (small["dtg"][0][:, 10:] == -1).all()


def _same_eval(ev, r, out, task):
    for k in ("precision", "recall", "scores"):
        assert ev.eval[task][k].shape == r.eval[k].shape and ev.eval[task][k].dtype == np.float64
        assert ev.eval[task][k].tobytes() == r.eval[k].tobytes(), (task, k)
    want = r.summarize()
    assert ev.stats[task].tobytes() == r.stats.tobytes()
    assert list(out[task]) == list(METRICS)
    for m in METRICS:
        assert (math.isnan(out[task][m]) and math.isnan(want[m])) or out[task][m] == want[m], (task, m)


def _feed(ev, dts):
    by = {}
    for d in dts:
        by.setdefault(d["image_id"], []).append(d)
    for i, ds in by.items():
        ev.process(i, ds)


def test_evaluator_end_to_end_and_ap_score_file(tmp_path):
    gt, dts = seeded_scene(7)                                           # six images, one category, crowds on images 3 and 6
    ev = coco_eval.COCOEvaluator(gt)
    _feed(ev, dts)
    out = ev.evaluate()
    assert sorted(out) == ["bbox", "segm"]
    for task in ("bbox", "segm"):
        _same_eval(ev, Restatement(gt, dts, task).evaluate().accumulate(), out, task)
    assert 5 < out["segm"]["AP"] < 95 and out["segm"]["AP"] != out["bbox"]["AP"]        # a scene that decides something
    # the same through the file interface: a predictions list with `weight` for `score`, ids missing
    gp, pp = tmp_path / "gt.json", tmp_path / "pred.json"
    gp.write_text(json.dumps(gt))
    pp.write_text(json.dumps([{("weight" if k == "score" else k): v for k, v in d.items()} for d in dts]))
    res = coco_eval.evaluate_ap(str(gp), str(pp), coco_eval.COCOEvaluator(str(gp)), str(tmp_path / "out"))
    written = json.loads((tmp_path / "out" / "ap_score.json").read_text())
    for task in ("bbox", "segm"):
        for m in METRICS:
            assert (math.isnan(written[task][m]) and math.isnan(out[task][m])) or written[task][m] == out[task][m] == res[task][m]
    assert written["number_of_images"] == 6 and written["number_of_annotations"] == len(dts)
    # a subset of the images
    ev.reset()
    _feed(ev, dts)
    sub = ev.evaluate(img_ids=[2, 3, 5])
    _same_eval(ev, Restatement(gt, dts, "segm", img_ids=[2, 3, 5]).evaluate().accumulate(), sub, "segm")


def test_evaluator_two_categories_limits_and_device_records():
    H, W = 64, 80
    rng = np.random.default_rng(17)
    gt, dts = seeded_scene(9, n_images=3, H=H, W=W, n_gt=4, n_noise=3)
    gt["categories"] = [{"id": 4, "name": "a"}, {"id": 2, "name": "b"}]
    for i, a in enumerate(gt["annotations"]):
        a["category_id"] = 4 if i % 3 else 2
    for i, d in enumerate(dts):
        d["category_id"] = 4 if i % 2 else 2
    gt["images"] += [{"id": 7, "height": H, "width": W, "file_name": "7.jpg"}, {"id": 8, "height": H, "width": W, "file_name": "8.jpg"},
                     {"id": 9, "height": H, "width": W, "file_name": "9.jpg"}]
    gt["annotations"] += [gt_ann(100, 7, blob(H, W, 20, 20, 8, 8), 4), gt_ann(101, 7, blob(H, W, 40, 50, 9, 12), 2)]      # image 7: no detection
    dts += [dt_ann(8, blob(H, W, 30, 30, 6, 9), 0.7, 2), dt_ann(8, blob(H, W, 10, 60, 5, 5), 0.7, 4)]                    # image 8: no ground truth
    gt["annotations"] += [gt_ann(102, 9, rect(H, W, 0, 0, 32, 32), 4), gt_ann(103, 9, rect(H, W, 0, 40, 32, 32), 4, area=9216.0)]    # 1024 and "9216"
    # image 9: 130 detections of one category made on the device; rle.encode's records go in unchanged
    masks = np.stack([blob(H, W, rng.uniform(0, 40), rng.uniform(0, W), rng.uniform(2, 20), rng.uniform(2, 20)) for _ in range(128)] +
                     [rect(H, W, 0, 0, 32, 32), rect(H, W, 0, 40, 32, 32)])
    recs = rle.encode(torch.from_numpy(masks).cuda())
    assert recs[128] == rle.encode_numpy(masks[128])
    for k, rec in enumerate(recs):
        dts.append({"image_id": 9, "category_id": 4, "score": float(np.round(rng.random(), 2)), "segmentation": rec, "bbox": rle.to_bbox(rec)})
    for max_dets, md in ((None, (1, 10, 100)), (120, (1, 10, 120))):
        ev = coco_eval.COCOEvaluator(gt, max_dets_per_image=max_dets)
        _feed(ev, dts)
        out = ev.evaluate()
        for task in ("bbox", "segm"):
            r = Restatement(gt, dts, task, max_dets=md).evaluate().accumulate()
            assert r.eval["precision"].shape == (10, 101, 2, 4, 3)
            _same_eval(ev, r, out, task)
