"""unmore_amd.rle.from_polygons on the device against the sequential restatement (rle.from_polygons_numpy, pinned by
tests/test_polygon_rle_cpu.py), and what is built on it: the evaluator's polygons="rasterize" and coco_eval.convert_polygons.  Every
comparison is of bytes or integers: there is no tolerance anywhere."""
import json

import numpy as np
import pytest
import torch

from unmore_amd import coco_eval, rle
from coco_eval_common import blob, dataset, dt_ann, gt_ann
from polygon_rle_common import ellipse, parity_mask, random_polygon, sweep

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (1, 9), (9, 1), (7, 5), (48, 64), (375, 500))


def _placed(rng, h, w, k, mode, place):
    """place 0: inside the image, 1: across its edges, 2: wholly outside it (shifted beyond the right and the bottom edge).  Up to
    three vertices lie anywhere; more form a jagged ring (the reference walks the outline point by point in Python: a ring keeps
    it to a few thousand points where 200 random vertices on 375 x 500 would make it 10^5)"""
    if k <= 3:
        xy = random_polygon(rng, h, w, k, mode, spread=0.0 if place != 1 else 0.4)
    else:
        grow = 0.35 if place != 1 else 0.7
        t = np.arange(k) * 2 * np.pi / k
        r = rng.uniform(0.6, 1.0, k)
        pts = np.stack([w / 2 + grow * w * r * np.cos(t), h / 2 + grow * h * r * np.sin(t)], axis=1)
        pts = np.round(pts) if mode == 0 else np.round(pts * 2) / 2 if mode == 1 else pts
        xy = [float(v) for v in pts.reshape(-1)]
    if place == 2:
        xy = [v + (1.5 * w + 3 if i % 2 == 0 else 1.5 * h + 3) for i, v in enumerate(xy)]
    return xy


def _check(segs, sizes):
    got = rle.from_polygons(segs, sizes)
    want = rle.from_polygons_numpy(segs, sizes)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g["size"], len(g["counts"]), len(w["counts"]))
    return got


def test_case_matrix_with_ragged_sizes_in_one_call():
    """every size x 1, 2, 3 and 200 vertices x integer, half-integer and random coordinates x inside, across, outside"""
    rng = np.random.default_rng(7)
    segs, sizes = [], []
    for h, w in SIZES:
        for k in (1, 2, 3, 200):
            for mode in range(3):
                for place in range(3):
                    segs.append([_placed(rng, h, w, k, mode, place)])
                    sizes.append((h, w))
    got = _check(segs, sizes)
    assert len(got) == 216 and [g["size"] for g in got] == [list(s) for s in sizes]
    full = [i for i, g in enumerate(got) if rle.area(g) > 0]
    assert len(full) > 40                                                     # the matrix is not a list of empty masks
    again = rle.from_polygons(segs, sizes)                                    # the same input gives the same bytes
    assert again == got
    one = rle.from_polygons([segs[-10]], sizes[-10])                          # one (H, W) for the call
    assert one == [got[-10]]


def test_many_polygons_overlapping_disjoint_duplicated_and_none():
    rng = np.random.default_rng(8)
    h, w = 48, 64
    seventy = [ellipse(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1, 9), rng.uniform(1, 9), int(rng.integers(3, 12))) for _ in range(70)]
    a, b, far = ellipse(20, 20, 12, 9, 16), ellipse(28, 24, 12, 9, 16, phase=0.3), ellipse(52, 38, 6, 5, 9)
    segs = [seventy, [a, b], [a, far], [a, a], [a, b, a, far, b], [], [a], [far, far, far]]
    got = _check(segs, (h, w))
    assert got[3] == got[6] and got[5]["counts"] == rle.counts_to_string([h * w])       # twice the same polygon: OR, not parity
    assert rle.area(got[1]) < rle.area(got[6]) + rle.area(rle.from_polygons_numpy([[b]], (h, w))[0])      # the overlap counts once
    masks = rle.decode(got)                                                   # end to end: the strings decode to the parity masks
    for m, seg in zip(masks, segs):
        assert (m.cpu().numpy() == 255 * parity_mask(seg, h, w)).all()


def test_sort_at_and_beyond_the_lds_capacity():
    """a sweep polyline of n edges over a 256-wide image has n * 256 crossings: exactly the LDS sort's capacity, two workgroups'
    worth beyond it, two short of it; and two polygons that fit one by one whose merged candidates do not"""
    cap = rle.POLY_SORT_LDS_KEYS
    h, w = 12, 256
    at, over = sweep(h, w, 16), sweep(h, w, 18)
    assert len(rle.polygon_crossings_numpy(at, h, w)) == cap and len(rle.polygon_crossings_numpy(over, h, w)) == cap + 512
    short = [0.7] + at[1:]                                                    # its first vertex lies right of column 0's centre line
    assert len(rle.polygon_crossings_numpy(short, h, w)) == cap - 2            # ... so the two edges that meet there miss that column
    half = sweep(h, w, 10)
    segs = [[at], [over], [short], [half, [v + 0.25 for v in half]], [over, at]]
    got = _check(segs, (h, w))
    assert rle.from_polygons(segs, (h, w)) == got


def test_strings_that_cross_the_back_end_chunk():
    """the back end takes 2 048 stream positions per chunk: outlines with more candidates than that, and more run boundaries"""
    rng = np.random.default_rng(9)
    segs = [[ellipse(250, 187, 240, 180, 120, wobble=6.0)],                       # ~ 960 candidates: inside one chunk
            [random_polygon(rng, 375, 500, 40, 2, spread=0.1)],                 # a star-like tangle: thousands of candidates
            [ellipse(250, 187, 240, 180, 90), ellipse(250, 187, 200, 150, 77), ellipse(100, 100, 90, 90, 50)]]
    got = _check(segs, (375, 500))
    assert len(rle.polygon_crossings_numpy(segs[1][0], 375, 500)) > 2 * 2048
    assert len(rle.string_to_counts(got[1]["counts"])) > 2049


def _polygon_dataset():
    """6 images of two sizes, 2 categories; ground truths as polygons (one or several per annotation), run-length records and crowds;
    detections = jittered ellipses with repeated scores.  Returns (gt with polygons, gt converted on the host, detections)"""
    rng = np.random.default_rng(10)
    images = [(i, 96, 128) if i % 2 else (i, 80, 100) for i in range(1, 7)]
    anns, dts, aid = [], [], 1
    for img, H, W in images:
        for k in range(5):
            cx, cy, rx, ry = rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(3, 35), rng.uniform(3, 28)
            cat = 1 + int(rng.integers(0, 2))
            kind = k % 3
            if kind == 0:                                                    # a polygon, sometimes in two parts
                seg = [ellipse(cx, cy, rx, ry, int(rng.integers(5, 40)), wobble=1.0)]
                if rng.random() < 0.5:
                    seg.append(ellipse(cx + rx, cy, rx / 2, ry / 2, 9))
                mask = parity_mask(seg, H, W)
            else:                                                            # a run-length record; every third one a crowd
                mask = blob(H, W, cy, cx, ry, rx)
                seg = None
            a = gt_ann(aid, img, mask, category_id=cat, iscrowd=int(kind == 2 and img % 2 == 0))
            if seg is not None:
                a["segmentation"] = seg
            anns.append(a)
            aid += 1
            if rng.random() < 0.85:
                j = rng.normal(0, 2.0, 4)
                dts.append(dt_ann(img, blob(H, W, cy + j[0], cx + j[1], max(ry + j[2], 1), max(rx + j[3], 1)), float(np.round(rng.random(), 1)), cat))
        for _ in range(3):
            dts.append(dt_ann(img, blob(H, W, rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, 20), rng.uniform(1, 20)),
                              float(np.round(rng.random(), 1)), 1 + int(rng.integers(0, 2))))
    gt = dataset(images, anns, categories=(1, 2))
    size_of = {i: (h, w) for i, h, w in images}
    host = dict(gt, annotations=[dict(a, segmentation=rle.from_polygons_numpy([a["segmentation"]], size_of[a["image_id"]])[0])
                                 if isinstance(a["segmentation"], list) else a for a in anns])
    return gt, host, dts


def _run(ev, dts):
    for d in dts:
        ev.process(d["image_id"], [d])
    return ev.evaluate()


def test_mask_iou_of_rasterised_polygons_equals_dense_numpy():
    h, w = 80, 100
    segs = [[ellipse(40, 30, 30, 20, 24)], [ellipse(50, 40, 30, 20, 17, wobble=2.0)], [ellipse(20, 60, 15, 15, 8), ellipse(70, 20, 25, 12, 30)]]
    recs = rle.from_polygons(segs, (h, w))
    dense = [parity_mask(s, h, w).astype(bool) for s in segs]
    crowd = [0, 1, 0]
    want = np.zeros((3, 3), np.float64)
    for d in range(3):
        for g in range(3):
            i = int((dense[d] & dense[g]).sum())
            u = int(dense[d].sum()) if crowd[g] else int(dense[d].sum()) + int(dense[g].sum()) - i
            want[d, g] = float(i) / float(u)
    got = coco_eval.mask_iou(recs, recs, crowd).cpu().numpy()
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()


def test_evaluator_rasterize_equals_the_host_conversion_and_convert_round_trips(tmp_path):
    gt, host, dts = _polygon_dataset()
    assert sum(isinstance(a["segmentation"], list) for a in gt["annotations"]) == 12 and any(a["iscrowd"] for a in gt["annotations"])
    with pytest.raises(ValueError, match="polygon"):                          # the default keeps raising
        _run(coco_eval.COCOEvaluator(gt), dts)
    ev_p, ev_h = coco_eval.COCOEvaluator(gt, polygons="rasterize"), coco_eval.COCOEvaluator(host)
    assert ev_p.gt["annotations"] == host["annotations"]                      # converted once, at construction: the same records
    res_p, res_h = _run(ev_p, dts), _run(ev_h, dts)
    for task in ("bbox", "segm"):
        assert ev_p.stats[task].tobytes() == ev_h.stats[task].tobytes()
        for k in ("precision", "recall", "scores"):
            assert ev_p.eval[task][k].tobytes() == ev_h.eval[task][k].tobytes(), (task, k)
        assert json.dumps(res_p[task]) == json.dumps(res_h[task])
    assert res_p["segm"]["AP"] > 5                                            # the detections do meet the polygons
    # the one-time file conversion
    src, dst = tmp_path / "gt.json", tmp_path / "gt_rle.json"
    src.write_text(json.dumps(gt))
    out = coco_eval.convert_polygons(str(src), str(dst))
    assert json.loads(dst.read_text()) == out == json.loads(json.dumps(host))
    assert all(a["area"] == b["area"] and a["bbox"] == b["bbox"] for a, b in zip(out["annotations"], gt["annotations"]))
    assert isinstance(json.loads(src.read_text())["annotations"][0]["segmentation"], list)      # the source file is left alone
    assert json.dumps(_run(coco_eval.COCOEvaluator(str(dst)), dts)["segm"]) == json.dumps(res_h["segm"])      # as text: nan is not == nan
