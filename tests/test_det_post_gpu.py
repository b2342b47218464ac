"""unmore_amd.detector_inference on the MI355X: one ragged batch through the selection against the restatement of
tests/det_post_common.py, the paste against torch's grid_sample in float64 by the band rule and against the restatement for equality,
the fused records against the unfused path character for character, and the fixture of the reference's own inference tail
(tests/golden/det_post.npz) on the device."""
import numpy as np
import pytest
import torch

import det_post_common as C

pytestmark = pytest.mark.gpu

F32 = np.float32
ROWS = (0, 1, 63, 65, 300, 1100)         # a 64-bit word, a 256-thread workgroup and 1024 are crossed
ST, NT = 0.05, 0.5


def _dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run_select(batch, topk, dev):
    from unmore_amd import detector_inference as D
    items, rows = D.fast_rcnn_inference([_t(b, dev) for b, _, _ in batch], [_t(s, dev) for _, s, _ in batch], [sh for _, _, sh in batch],
                                        ST, NT, topk)
    return [(it["pred_boxes"].cpu().numpy(), it["scores"].cpu().numpy(), it["pred_classes"].cpu().numpy(), r.cpu().numpy())
            for it, r in zip(items, rows)]


@pytest.fixture(scope="module")
def selection():
    """the one device run the selection tests share: K = 1 with class-agnostic boxes and K = 3 with class-specific [R, 12] boxes, each
    at topk -1, 7 and 5000; the restatement once, at topk -1 (a top-k cut is a prefix of it)"""
    dev = _dev()
    out = {}
    for K, specific in ((1, False), (3, True)):
        batch = C.selection_batch(5, K, specific, ROWS)
        want = [C.select_numpy(b, s, sh, ST, NT, -1) for b, s, sh in batch]
        out[K] = (batch, want, {topk: _run_select(batch, topk, dev) for topk in (-1, 7, 5000)})
    return out


@pytest.mark.parametrize("K", [1, 3])
def test_selection_equals_the_restatement(selection, K):
    batch, want, got = selection[K]
    counts = [len(w[0]) for w in want]
    print("kept per image:", counts, "of", [len(b) * K for b, _, _ in batch])
    assert counts[0] == 0 and counts[2] == 0 and counts[1] >= 1              # no rows; nothing passes the threshold
    assert counts[5] > 7 and counts[5] < 1100 * K                            # topk 7 cuts, 5000 does not; NMS removed a fair share
    for topk, res in got.items():
        for k, (w, g) in enumerate(zip(want, res)):
            n = len(w[0]) if topk < 0 else min(len(w[0]), topk)
            assert len(g[0]) == n, (topk, k)
            assert np.array_equal(g[3], w[3][:n]) and np.array_equal(g[2], w[2][:n]), (topk, k)          # rows and classes
            assert g[0].tobytes() == w[0][:n].tobytes() and g[1].tobytes() == w[1][:n].tobytes(), (topk, k)
            assert g[2].dtype == np.int64 and g[3].dtype == np.int64 and g[0].dtype == F32
    # the planted cases, in the image with 300 rows
    b, s, c, rows = want[4]
    kept = set(zip(rows.tolist(), c.tolist()))
    assert (0, 0) in kept and (1, 0) in kept                                  # IoU exactly 0.5 suppresses nothing at 0.5
    assert (2, 0) in kept and (3, 0) not in kept                              # the duplicated box
    assert not {40, 41, 42, 43} & set(rows.tolist())                          # NaN / inf in a box or a score
    assert {(44, 0), (45, 0), (46, 0)} <= kept                                # zero area after the clip: suppress nothing
    assert (50, 0) not in kept                                                # a score equal to the threshold
    ties = [r for r, cl in zip(rows.tolist(), c.tolist()) if cl == 0 and 10 <= r < 20]
    assert ties == sorted(ties) and len(ties) >= 2                            # equal scores keep candidate order


def test_selection_same_bytes_and_limit(selection):
    from unmore_amd import _lib, detector_inference as D
    dev = _dev()
    batch, _, got = selection[3]
    again = _run_select(batch, -1, dev)
    for a, b in zip(got[-1], again):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    before = _lib._count[0]
    with pytest.raises(ValueError, match="at most 8192"):
        D.fast_rcnn_inference([torch.zeros((8193, 4), device=dev)], [torch.zeros((8193, 2), device=dev)], [(10, 10)], 0.0, 0.5, 100)
    assert _lib._count[0] == before                                           # no launch
    items, rows = D.fast_rcnn_inference([torch.zeros((0, 4), device=dev)], [torch.zeros((0, 2), device=dev)], [(10, 10)], 0.0, 0.5, 100)
    assert len(items) == 1 and items[0]["pred_boxes"].shape == (0, 4) and rows[0].numel() == 0


def test_selection_fixture_on_the_device():
    from unmore_amd import detector_inference as D
    dev = _dev()
    fx = C.load_fixture()
    N = int(fx["n_images"])
    items, rows = D.fast_rcnn_inference([_t(fx[f"im{k}_boxes"], dev) for k in range(N)], [_t(fx[f"im{k}_scores"], dev) for k in range(N)],
                                        [tuple(v) for v in fx["in_sizes"].tolist()], float(fx["score_thresh"]), float(fx["nms_thresh"]),
                                        int(fx["topk"]))
    for k in range(N):
        assert np.array_equal(rows[k].cpu().numpy(), fx[f"im{k}_kept"]), k
        assert np.array_equal(items[k]["pred_classes"].cpu().numpy(), fx[f"im{k}_pred_classes"])
        assert items[k]["pred_boxes"].cpu().numpy().tobytes() == fx[f"im{k}_pred_boxes"].tobytes()
        assert items[k]["scores"].cpu().numpy().tobytes() == fx[f"im{k}_pred_scores"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the shared scan
def _same(got, want, n=None):
    """a device result (boxes, scores, classes, rows) equals the first n entries of a restatement's or of another device result"""
    n = len(want[0]) if n is None else n
    return (len(got[0]) == n and np.array_equal(got[3], want[3][:n]) and np.array_equal(got[2], want[2][:n]) and
            got[0].tobytes() == want[0][:n].tobytes() and got[1].tobytes() == want[1][:n].tobytes())


@pytest.mark.parametrize("R,K", [(4097, 1), (4096, 2)])
def test_selection_with_two_removed_words_per_lane(R, K):
    """4097 candidates, the first count that needs the second word of removed set per lane, and 8192, the table's maximum; several
    hundred survive per class, past rank 4096 too; the cut at 100 is a prefix"""
    dev = _dev()
    batch = [C.many_candidates(R, K)]
    want = C.select_numpy(*batch[0], ST, NT, -1)
    print("kept", len(want[0]), "of", R * K)
    assert R * K > 4096 and 300 < len(want[0]) < R * K // 2
    assert _same(_run_select(batch, -1, dev)[0], want)
    assert _same(_run_select(batch, 100, dev)[0], want, 100)


def test_selection_on_the_constructed_blocks():
    """tests/nms_cases.py: chains inside a 64-rank block, into the next and over a wholly suppressed one, a block of duplicates, two
    zero-area boxes; test_det_post_cpu.py checks that the restatement gives the constructed list"""
    import nms_cases as NC
    dev = _dev()
    batch = [C.ranked_image(NC.constructed_boxes()[0])]
    got = _run_select(batch, -1, dev)[0]
    assert _same(got, C.select_numpy(*batch[0], ST, NC.THRESH, -1))
    NC.check_expected(got[3])


@pytest.fixture(scope="module")
def limited():
    """the constructed image (193 kept of 322) and one of 30 separate boxes, whose cap min(P, topk) = 30 is below every topk from 63 on"""
    import nms_cases as NC
    dev = _dev()
    batch = [C.ranked_image(NC.constructed_boxes()[0]), C.ranked_image(NC.line_boxes(128 * np.arange(30)))]
    return {topk: _run_select(batch, topk, dev) for topk in (-1, 0, 1, 63, 64, 65, 128)}


@pytest.mark.parametrize("topk", [0, 1, 63, 64, 65, 128])
def test_selection_limit_is_a_prefix(limited, topk):
    """63 ranks are kept in the first block of 64: a limit of 63 ends the walk there, 64 and 65 end it inside the second block"""
    full = limited[-1]
    assert len(full[0][0]) > 130 and len(full[1][0]) == 30
    assert _same(limited[topk][0], full[0], topk)                              # counts == topk
    assert _same(limited[topk][1], full[1], min(topk, 30))                     # cap < topk


@pytest.mark.parametrize("specific", [False, True])
def test_selection_class_predicate(specific):
    """the same box under two classes is kept twice, under one class once"""
    dev = _dev()
    batch = C.class_pairs(specific)
    got = _run_select(batch, -1, dev)
    for g, (b, s, sh), kept in zip(got, batch, C.CLASS_PAIRS_KEPT):
        assert _same(g, C.select_numpy(b, s, sh, ST, NT, -1))
        assert list(zip(g[3].tolist(), g[2].tolist())) == kept


# ---------------------------------------------------------------------------------------------------------------- the paste
PASTE_CASES = ((28, 1, 96, 130, False), (7, 3, 37, 53, False), (28, 3, 37, 53, True), (7, 1, 96, 130, False))


@pytest.fixture(scope="module")
def pasted():
    """one device run per (M, C, frame): smooth logits, boxes of at least 4 px per side; bfloat16 logits for one image"""
    from unmore_amd import detector_inference as D
    dev = _dev()
    out = []
    for M, Cn, H, W, bf16 in PASTE_CASES:
        rng = np.random.RandomState(100 + M + Cn + H)
        n = 16
        logits = C.smooth_logits(rng, n, Cn, M)
        boxes = C.random_boxes(rng, n, H, W)
        classes = rng.randint(Cn, size=n).astype(np.int64)
        lt = _t(logits, dev)
        if bf16:
            lt = lt.to(torch.bfloat16)
            logits = lt.float().cpu().numpy()
        got = D.paste_masks(lt, _t(boxes, dev), _t(classes, dev) if Cn > 1 else None, H, W)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, H, W)
        out.append((M, Cn, H, W, bf16, logits, boxes, classes, got.cpu().numpy()))
    return out


@pytest.mark.parametrize("case", range(len(PASTE_CASES)))
def test_paste_against_grid_sample_by_the_band_rule(pasted, case):
    M, Cn, H, W, bf16, logits, boxes, classes, got = pasted[case]
    assert got.max() == 1 and 0 < got.sum() < got.size
    prob = C.probs_numpy(logits, classes)
    C.band_check(got, prob, boxes, H, W, what=f"device, M={M} C={Cn} {H}x{W}{' bf16' if bf16 else ''}")


def test_paste_edge_cases_equal_the_restatement():
    from unmore_amd import detector_inference as D
    dev = _dev()
    rng = np.random.RandomState(21)
    H, W, M = 37, 53, 28
    boxes = np.array([[0, 0, W, H],                    # the whole frame
                      [0, 5.5, 20.25, 30],             # flush with the left edge
                      [30.5, 0, 50, 12.75],            # the top
                      [33.3, 10, W, 31.2],             # the right
                      [12, 20.6, 40, H],               # the bottom
                      [-20.5, -10.25, 21.5, 17.75],    # half outside before the clip
                      [40.2, 25.1, 70.9, 52.3],
                      [10, 10, 11, 11],                # one pixel
                      [10.3, 10.6, 11.3, 11.6],        # one pixel across pixel borders
                      [20.4, 8.1, 20.9, 8.7],          # sub-pixel, around a pixel centre
                      [20.6, 8.6, 20.9, 8.9],          # sub-pixel, no centre inside
                      [5, 5, 5, 9], [9, 5, 5, 9],      # empty and inverted
                      [60, 40, 80, 50],                # outside the frame
                      [3.2, 2.5, 17.8, 11.1], [3.2, 2.5, 17.8, 11.1]], dtype=F32)
    n = len(boxes)
    logits = C.smooth_logits(rng, n, 1, M)
    logits[-2], logits[-1] = -4.0, 9.0                 # all-negative and all-positive logits
    got = D.paste_masks(_t(logits, dev), _t(boxes, dev), None, H, W).cpu().numpy()
    want = C.paste_masks_numpy(logits, boxes, None, H, W)
    for k in range(n):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    assert not got[-2].any() and got[-1, 3:11, 4:17].all() and not got[11:14].any()
    # the two dyadic hand cases: weights 1 / 0, and 1/4 / 3/4
    Ms = 7
    lg = (rng.standard_normal((2, 1, Ms, Ms)) * 3).astype(F32)
    a = D.paste_masks(_t(lg[:1], dev), _t(np.array([[0, 0, Ms, Ms]], F32), dev), None, Ms, Ms).cpu().numpy()[0]
    assert np.array_equal(a, C.sigmoid_f32(lg[0, 0]) >= 0.5)
    b = D.paste_masks(_t(lg[1:], dev), _t(np.array([[0, 0, 2 * Ms, 2 * Ms]], F32), dev), None, 2 * Ms, 2 * Ms).cpu().numpy()[0]
    assert np.array_equal(b, C.paste_numpy(C.sigmoid_f32(lg[1, 0]), [0, 0, 2 * Ms, 2 * Ms], 2 * Ms, 2 * Ms))
    # a threshold above 1/2
    c = D.paste_masks(_t(logits[:2], dev), _t(boxes[:2], dev), None, H, W, threshold=0.75).cpu().numpy()
    assert np.array_equal(c, C.paste_masks_numpy(logits[:2], boxes[:2], None, H, W, 0.75))


# ---------------------------------------------------------------------------------------------------------------- the records
@pytest.fixture(scope="module")
def records():
    """a three-image batch: ratios 2x exactly (48x65 -> 96x130) and non-integer (50x67 -> 37x53), one image without detections, one
    box that is empty after scale and clip; class-specific float32 logits with C = 2"""
    from unmore_amd import detector_inference as D
    dev = _dev()
    rng = np.random.RandomState(33)
    in_sizes, out_sizes, ids = [(48, 65), (40, 60), (50, 67)], [(96, 130), (80, 120), (37, 53)], [7, 8, 9]
    def inside(n, h, w):                                # boxes inside the frame, a third to a half of it per side
        x0, y0 = rng.uniform(0, 0.4 * w, n), rng.uniform(0, 0.4 * h, n)
        return np.stack([x0, y0, x0 + rng.uniform(0.3, 0.55, n) * w, y0 + rng.uniform(0.3, 0.55, n) * h], axis=1).astype(F32)
    boxes = [inside(6, 48, 65), np.zeros((0, 4), F32), inside(5, 50, 67)]
    boxes[2][1] = [70, 5, 80, 20]                       # right of the 67-wide frame: zero width after the clip to 53
    scores = [np.sort(rng.uniform(0.1, 1, len(b)).astype(F32))[::-1].copy() for b in boxes]
    classes = [rng.randint(2, size=len(b)).astype(np.int64) for b in boxes]
    n = sum(len(b) for b in boxes)
    logits = C.blob_logits(rng, n, 2, 28)
    dets = [{"pred_boxes": _t(b, dev), "scores": _t(s, dev), "pred_classes": _t(c, dev)} for b, s, c in zip(boxes, scores, classes)]
    cats = {0: 1, 1: 3}
    got = D.coco_records(dets, _t(logits, dev), in_sizes, out_sizes, ids, category_ids=cats)
    bare = D.coco_records(dets, None, in_sizes, out_sizes, ids, category_ids=cats)
    return dict(boxes=boxes, scores=scores, classes=classes, logits=logits, in_sizes=in_sizes, out_sizes=out_sizes, ids=ids, cats=cats, got=got,
                bare=bare)


def test_records_fields_and_strings(records):
    from unmore_amd import detector_inference as D, rle
    dev = _dev()
    r = records
    want = C.records_numpy(list(zip(r["boxes"], r["scores"], r["classes"])), None, r["in_sizes"], r["out_sizes"], r["ids"], r["cats"])
    assert [len(x) for x in r["got"]] == [6, 0, 4] and r["got"][1] == []      # no detections; the empty box's record is absent
    at = 0
    for k, (mine, bare, ref) in enumerate(zip(r["got"], r["bare"], want)):
        assert len(mine) == len(bare) == len(ref)
        b, keep = C.postprocess_numpy(r["boxes"][k], r["in_sizes"][k], r["out_sizes"][k])
        n = len(b)
        if n:
            H, W = r["out_sizes"][k]
            frames = D.paste_masks(_t(r["logits"][at:at + n], dev), _t(b, dev), _t(r["classes"][k], dev), H, W)
            strings = [s for s, kp in zip(rle.encode(frames), keep) if kp]
        for i, (m, bb, rf) in enumerate(zip(mine, bare, ref)):
            assert list(m) == ["image_id", "category_id", "bbox", "score", "segmentation"] and list(bb) == list(m)[:4]
            assert {x: m[x] for x in list(m)[:4]} == rf == bb                 # bbox and score: the restatement's floats, exactly
            assert type(m["score"]) is float and all(type(v) is float for v in m["bbox"]) and type(m["category_id"]) is int
            assert m["segmentation"] == strings[i], (k, i)                     # character for character: no band between fused and unfused
            assert rle.area(m["segmentation"]) > 0
        at += n


def test_records_through_the_evaluator(records):
    from unmore_amd import rle
    from unmore_amd.coco_eval import COCOEvaluator
    r = records
    gt = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in zip(r["ids"], r["out_sizes"])],
          "categories": [{"id": 1}, {"id": 3}], "annotations": []}
    for recs in r["got"]:
        for rec in recs:
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": rec["image_id"], "category_id": rec["category_id"],
                                      "bbox": list(rec["bbox"]), "area": float(rle.area(rec["segmentation"])), "iscrowd": 0,
                                      "segmentation": dict(rec["segmentation"])})
    ev = COCOEvaluator(gt)
    for i, recs in zip(r["ids"], r["got"]):
        ev.process(i, recs)                                                   # unchanged
    out = ev.evaluate()
    assert out["segm"]["AP"] == 100.0 and out["bbox"]["AP"] == 100.0


def test_records_fixture_on_the_device():
    from unmore_amd import detector_inference as D, rle
    dev = _dev()
    fx = C.load_fixture()
    N = int(fx["n_images"])
    in_sizes, out_sizes = [tuple(v) for v in fx["in_sizes"].tolist()], [tuple(v) for v in fx["out_sizes"].tolist()]
    dets = [{"pred_boxes": _t(fx[f"im{k}_pred_boxes"], dev), "scores": _t(fx[f"im{k}_pred_scores"], dev),
             "pred_classes": _t(fx[f"im{k}_pred_classes"], dev)} for k in range(N)]
    got = D.coco_records(dets, _t(fx["mask_logits"], dev), in_sizes, out_sizes, [100 + k for k in range(N)])
    at = 0
    for k in range(N):
        mine = got[k]
        assert len(mine) == int(fx[f"im{k}_rec_n"])
        assert np.array_equal(np.array([r["bbox"] for r in mine]).reshape(-1, 4), fx[f"im{k}_rec_bbox"])
        assert np.array_equal(np.array([r["score"] for r in mine]), fx[f"im{k}_rec_score"])
        assert [r["category_id"] for r in mine] == fx[f"im{k}_rec_category"].tolist() and all(r["image_id"] == 100 + k for r in mine)
        b, keep = C.postprocess_numpy(fx[f"im{k}_pred_boxes"], in_sizes[k], out_sizes[k])
        probs = C.probs_numpy(fx["mask_logits"][at:at + len(keep)], fx[f"im{k}_pred_classes"])[keep]
        masks = np.stack([m.cpu().numpy() != 0 for m in rle.decode([r["segmentation"] for r in mine], device=dev)])
        C.band_check(masks, probs, b[keep], *out_sizes[k], what=f"device records, image {k}")
        same = sum(r["segmentation"]["counts"] == w.decode("ascii") for r, w in zip(mine, fx[f"im{k}_rec_counts"]))
        print(f"image {k}: {same} of {len(mine)} strings equal the reference's")
        at += len(keep)
