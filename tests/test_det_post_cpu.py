"""unmore_amd.detector_inference without a GPU: the restatement (tests/det_post_common.py) against the fixture the reference's own
inference tail wrote (tests/golden/make_golden_det_post.py), hand-worked NMS and paste cases through the restatement, the written-out
paste against torch's F.grid_sample, the C-ABI entries' argument checks and the argument errors of the Python entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import det_post_common as C
from unmore_amd import rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("umr_det_select_workspace", "umr_det_select", "umr_det_scale", "umr_det_paste", "umr_det_paste_rle")
F32 = np.float32


def _select(boxes, scores, shape=(100, 100), st=0.05, nt=0.5, topk=-1):
    scores = np.asarray(scores, F32)
    if scores.ndim == 1:
        scores = np.stack([scores, 1 - scores], axis=1)
    return C.select_numpy(np.asarray(boxes, F32), scores, shape, st, nt, topk)


def test_restatement_reproduces_the_fixture():
    """The reference's own flow: kept indices, classes and record fields equal, boxes and scores bit-equal, mask strings equal except
    as the band rule allows."""
    fx = C.load_fixture()
    N = int(fx["n_images"])
    st, nt, topk = float(fx["score_thresh"]), float(fx["nms_thresh"]), int(fx["topk"])
    items, at, dropped = [], 0, 0
    for k in range(N):
        b, s, c, rows = C.select_numpy(fx[f"im{k}_boxes"], fx[f"im{k}_scores"], tuple(fx["in_sizes"][k]), st, nt, topk)
        assert np.array_equal(rows, fx[f"im{k}_kept"]) and np.array_equal(c, fx[f"im{k}_pred_classes"]), k
        assert b.tobytes() == fx[f"im{k}_pred_boxes"].tobytes() and s.tobytes() == fx[f"im{k}_pred_scores"].tobytes(), k
        assert len(b) == topk                                                   # the top-k cut is exercised
        items.append((b, s, c))
    in_sizes, out_sizes = [tuple(v) for v in fx["in_sizes"].tolist()], [tuple(v) for v in fx["out_sizes"].tolist()]
    recs = C.records_numpy(items, fx["mask_logits"], in_sizes, out_sizes, [100 + k for k in range(N)])
    for k in range(N):
        mine = recs[k]
        assert len(mine) == int(fx[f"im{k}_rec_n"])
        dropped += len(items[k][0]) - len(mine)
        assert all(list(r) == ["image_id", "category_id", "bbox", "score", "segmentation"] and r["image_id"] == 100 + k for r in mine)
        assert np.array_equal(np.array([r["bbox"] for r in mine]).reshape(-1, 4), fx[f"im{k}_rec_bbox"])          # floats of float32: exact
        assert np.array_equal(np.array([r["score"] for r in mine]), fx[f"im{k}_rec_score"])
        assert np.array_equal(np.array([r["category_id"] for r in mine], dtype=np.int64), fx[f"im{k}_rec_category"])
        want = [c.decode("ascii") for c in fx[f"im{k}_rec_counts"]]
        b, keep = C.postprocess_numpy(items[k][0], in_sizes[k], out_sizes[k])
        probs = C.probs_numpy(fx["mask_logits"][at:at + len(keep)], items[k][2])[keep]
        differ = [i for i, r in enumerate(mine) if r["segmentation"]["counts"] != want[i]]
        assert all(r["segmentation"]["size"] == list(out_sizes[k]) for r in mine)
        if differ:                                                              # only inside the band around the threshold
            got = np.stack([rle.decode_numpy(r["segmentation"]) for r in mine])
            ref = np.stack([rle.decode_numpy({"size": list(out_sizes[k]), "counts": w}) for w in want])
            C.band_check(got, probs, b[keep], *out_sizes[k], what=f"restatement, image {k}")
            C.band_check(ref, probs, b[keep], *out_sizes[k], what=f"fixture, image {k}")
        at += len(keep)
    assert dropped == 1                                                         # the box that became empty after scale and clip


def test_nms_hand_cases():
    pair = [[0, 0, 3, 1], [1, 0, 4, 1]]                                         # inter 2, union 4: IoU exactly 0.5
    assert C.iou_f32(pair[0], pair[1]) == F32(0.5)
    assert list(_select(pair, [0.9, 0.8], nt=0.5)[3]) == [0, 1]                 # 0.5 > 0.5 is false: both kept
    assert list(_select(pair, [0.9, 0.8], nt=0.49)[3]) == [0]
    assert list(_select(pair, [0.8, 0.9], nt=0.49)[3]) == [1]
    dup = [[10, 10, 20, 20], [10, 10, 20, 20], [50, 50, 60, 60]]
    assert list(_select(dup, [0.7, 0.9, 0.8])[3]) == [1, 2]                     # a duplicated box: the higher score stays
    assert list(_select(dup, [0.7, 0.7, 0.7])[3]) == [0, 2]                     # equal scores keep candidate order
    sep = [[0, 0, 10, 10], [30, 0, 40, 10], [60, 0, 70, 10]]
    assert list(_select(sep, [0.6, 0.6, 0.6], topk=2)[3]) == [0, 1]
    # different classes never suppress each other
    boxes = np.array([[10, 10, 20, 20], [10, 10, 20, 20]], F32)
    scores = np.array([[0.6, 0.1, 0.3], [0.1, 0.7, 0.2]], F32)
    b, s, c, rows = C.select_numpy(boxes, scores, (100, 100), 0.05, 0.5, -1)
    assert list(zip(rows, c)) == [(1, 1), (0, 0)]                               # 0.7, 0.6; the two 0.1s are suppressed by their own class
    scores = np.array([[0.6, 0.1, 0.3], [0.5, 0.3, 0.2]], F32)
    assert list(zip(*C.select_numpy(boxes, scores, (100, 100), 0.2, 0.5, -1)[2:][::-1])) == [(0, 0), (1, 1)]
    # class-specific boxes: columns 4c .. 4c + 3
    boxes = np.array([[0, 0, 10, 10, 50, 50, 60, 60]], F32)
    b, s, c, rows = C.select_numpy(boxes, np.array([[0.5, 0.4, 0.1]], F32), (100, 100), 0.05, 0.5, -1)
    assert np.array_equal(b, [[0, 0, 10, 10], [50, 50, 60, 60]]) and list(c) == [0, 1]
    # a score equal to the threshold is dropped
    assert list(_select(sep, [F32(0.05), 0.06, 0.04])[3]) == [1]
    # a zero-area clipped box suppresses nothing (0 / 0 is NaN) and is kept
    out = [[120, 5, 140, 15], [125, 6, 150, 18], [0, 0, 10, 10]]
    b, s, c, rows = _select(out, [0.9, 0.8, 0.7])
    assert list(rows) == [0, 1, 2] and np.array_equal(b[0], [100, 5, 100, 15]) and np.isnan(C.iou_f32(b[0], b[1]))
    # rows with a non-finite entry are dropped, the background column included
    bad = np.array([[0, 0, 10, 10], [np.nan, 0, 10, 10], [30, 0, 40, np.inf], [60, 0, 70, 10]], F32)
    sc = np.array([[0.9, 0.1], [0.9, 0.1], [0.9, 0.1], [0.9, np.nan]], F32)
    assert list(C.select_numpy(bad, sc, (100, 100), 0.05, 0.5, -1)[3]) == [0]


def test_paste_hand_cases():
    rng = np.random.RandomState(3)
    M = 7
    prob = C.sigmoid_f32(rng.standard_normal((M, M)) * 3)
    # box [0, 0, M, M] on an M x M frame: every pixel centre is a tap, weights 1 and 0
    assert np.array_equal(C.paste_numpy(prob, [0, 0, M, M], M, M), prob >= 0.5)
    # box [0, 0, 2M, 2M] on a 2M x 2M frame: ix = (x + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, ...: weights 3/4 and 1/4, zero padding outside
    pad = np.zeros((M + 2, M + 2), F32)
    pad[1:-1, 1:-1] = prob
    want = np.zeros((2 * M, 2 * M), np.uint8)
    for y in range(2 * M):
        for x in range(2 * M):
            yl, xl = (y + 1) // 2 - 1, (x + 1) // 2 - 1                         # floor(y / 2 - 0.25)
            wy1, wx1 = (F32(0.75), F32(0.25))[y % 2], (F32(0.75), F32(0.25))[x % 2]
            wy0, wx0 = F32(1) - wy1, F32(1) - wx1
            v = F32(F32(F32(wx0 * wy0) * pad[yl + 1, xl + 1] + F32(wx1 * wy0) * pad[yl + 1, xl + 2]) + F32(wx0 * wy1) * pad[yl + 2, xl + 1])
            want[y, x] = F32(v + F32(wx1 * wy1) * pad[yl + 2, xl + 2]) >= 0.5
    got = C.paste_numpy(prob, [0, 0, 2 * M, 2 * M], 2 * M, 2 * M)
    assert np.array_equal(got, want) and 0 < got.sum() < got.size
    # all-negative logits give the empty string, all-positive ones the box
    neg = C.paste_masks_numpy(np.full((1, 1, M, M), -4, F32), [[3.2, 2.5, 17.8, 11.1]], None, 13, 21)[0]
    assert rle.encode_numpy(neg)["counts"] == rle.encode_numpy(np.zeros((13, 21), np.uint8))["counts"] and not neg.any()
    pos = C.paste_masks_numpy(np.full((1, 1, M, M), 9, F32), [[3.0, 2.0, 17.0, 11.0]], None, 13, 21)[0]
    box = np.zeros((13, 21), np.uint8)
    box[2:11, 3:17] = 1
    assert np.array_equal(pos, box)
    # degenerate boxes set nothing
    for b in ([5, 5, 5, 9], [5, 5, 9, 5], [9, 5, 5, 9], [np.nan, 0, 4, 4], [0, 0, np.inf, 4], [30, 2, 40, 9]):
        assert not C.paste_numpy(prob, b, 13, 21).any()
    # class-specific logits read the predicted class's channel
    lg = np.stack([np.full((M, M), -4, F32), np.full((M, M), 9, F32)])[None]
    assert not C.paste_masks_numpy(lg, [[0, 0, 5, 5]], [0], 8, 8).any() and C.paste_masks_numpy(lg, [[0, 0, 5, 5]], [1], 8, 8)[0, :5, :5].all()


@pytest.mark.parametrize("M,H,W", [(28, 96, 130), (7, 37, 53)])
def test_written_out_paste_against_grid_sample(M, H, W):
    """the NumPy float32 paste against torch's F.grid_sample as _do_paste_mask calls it, by the band rule; torch's own float32 too"""
    rng = np.random.RandomState(11 + M)
    n = 12
    logits = C.smooth_logits(rng, n, 1, M)
    boxes = C.random_boxes(rng, n, H, W)
    prob = C.probs_numpy(logits, None)
    got = np.stack([C.paste_numpy(prob[k], boxes[k], H, W) for k in range(n)])
    assert got.any()
    C.band_check(got, prob, boxes, H, W, what=f"numpy float32, M={M}")
    C.band_check(C.paste_torch(prob, boxes, H, W) >= 0.5, prob, boxes, H, W, what=f"torch float32, M={M}")


def test_records_restatement_fields():
    items = [(np.array([[2, 3, 30, 20], [60, 2, 64, 8]], F32), np.array([0.75, 0.5], F32), np.array([0, 1])), (np.zeros((0, 4), F32),) * 3]
    recs = C.records_numpy(items, None, [(48, 65), (50, 67)], [(96, 130), (37, 53)], ["a", 7], category_ids={0: 11, 1: 22})
    assert recs[1] == [] and [r["category_id"] for r in recs[0]] == [11, 22]
    assert recs[0][0] == {"image_id": "a", "category_id": 11, "bbox": [4.0, 6.0, 56.0, 34.0], "score": 0.75}
    assert all(type(v) is float for r in recs[0] for v in r["bbox"] + [r["score"]])
    assert C.scale_ratio(53, 67) == F32(53 / 67) and float(C.scale_ratio(130, 65)) == 2.0


def test_new_exports_are_declared_bound_and_check_their_arguments():
    from unmore_amd import _lib
    with open(os.path.join(ROOT, "include", "umr.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(umr_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None
    assert "csrc/det_post.hip" in hdr and ctypes.sizeof(_lib.DpImage) == 48 and _lib.DpImage.width.offset == 44
    assert lib.umr_det_select_workspace(-1, 1, 1) == -1 and lib.umr_det_select_workspace(1, -1, 1) == -1
    assert lib.umr_det_select_workspace(2, 100, 200) == 16 + 100 * 16 + 2 * 400 + 200 * 8
    vp, f32 = ctypes.c_void_p, _lib.F32
    p = vp(16)
    big = 1 << 20
    calls = (
        lambda: lib.umr_det_select(None, 1, 1, 1, 10, 10, 10, 10, 0.0, 0.5, -1, 7, p, p, p, p, p, p, big, None),          # a null table
        lambda: lib.umr_det_select(p, 0, 1, 1, 10, 10, 10, 10, 0.0, 0.5, -1, 7, p, p, p, p, p, p, big, None),
        lambda: lib.umr_det_select(p, 1, 0, 1, 10, 10, 10, 10, 0.0, 0.5, -1, 7, p, p, p, p, p, p, big, None),             # no class
        lambda: lib.umr_det_select(p, 1, 3, 2, 10, 10, 10, 10, 0.0, 0.5, -1, 7, p, p, p, p, p, p, big, None),             # boxes for 2 of 3 classes
        lambda: lib.umr_det_select(p, 1, 1, 1, 8193, 8193, 10, 10, 0.0, 0.5, -1, 7, p, p, p, p, p, p, 1 << 30, None),     # 8193 pairs
        lambda: lib.umr_det_select(p, 1, 1, 1, 10, 10, 10, 10, float("nan"), 0.5, -1, 7, p, p, p, p, p, p, big, None),
        lambda: lib.umr_det_select(p, 1, 1, 1, 10, 10, 10, 10, 0.0, float("nan"), -1, 7, p, p, p, p, p, p, big, None),
        lambda: lib.umr_det_select(p, 1, 1, 1, 10, 10, 10, 10, 0.0, 0.5, -1, 7, None, p, p, p, p, p, big, None),          # a null output
        lambda: lib.umr_det_select(p, 1, 1, 1, 10, 10, 10, 10, 0.0, 0.5, -1, 7, p, p, p, p, p, vp(8), big, None),         # misaligned workspace
        lambda: lib.umr_det_select(p, 1, 1, 1, 10, 10, 10, 10, 0.0, 0.5, -1, 7, p, p, p, p, p, p, 64, None),              # an undersized workspace
        lambda: lib.umr_det_select(p, 1, 1, 1, 10, 10, 10, 11, 0.0, 0.5, -1, 7, p, p, p, p, p, p, big, None),             # more slots than pairs
        lambda: lib.umr_det_scale(None, p, 3, p, None),
        lambda: lib.umr_det_scale(p, p, 0, p, None),
        lambda: lib.umr_det_paste(None, f32, 1, 1, 28, None, p, 4, 8, 8, 0.5, p, None),
        lambda: lib.umr_det_paste(p, 7, 1, 1, 28, None, p, 4, 8, 8, 0.5, p, None),                                        # an unknown dtype
        lambda: lib.umr_det_paste(p, f32, 1, 3, 28, None, p, 4, 8, 8, 0.5, p, None),                                      # classes missing
        lambda: lib.umr_det_paste(p, f32, 1, 1, 129, None, p, 4, 8, 8, 0.5, p, None),                                     # M > 128
        lambda: lib.umr_det_paste(p, f32, 1, 1, 28, None, p, 4, 8, 8, 0.25, p, None),                                     # threshold < 0.5
        lambda: lib.umr_det_paste(p, f32, 1, 1, 28, None, p, 4, 1 << 16, 1 << 16, 0.5, p, None),                          # H * W >= 2^31
        lambda: lib.umr_det_paste(p, f32, 1, 1, 28, None, p, 3, 8, 8, 0.5, p, None),
        lambda: lib.umr_det_paste_rle(p, f32, 1, 1, 28, None, p, 4, None, 2, 0.5, p, None, None, 0, None),                # no frames
        lambda: lib.umr_det_paste_rle(p, f32, 1, 1, 28, None, p, 4, p, 2, 0.5, None, None, None, 0, None),                # no sizes
        lambda: lib.umr_det_paste_rle(p, f32, 1, 1, 28, None, p, 4, p, 2, 0.5, None, None, p, 10, None),                  # chars without offsets
    )
    for k, call in enumerate(calls):
        assert call() != 0, k
        assert lib.umr_last_error_string()


def test_argument_errors_and_no_cpu_fallback():
    from unmore_amd import detector_inference as D
    b, s = torch.zeros((5, 4)), torch.full((5, 2), 0.5)
    for call in (lambda: D.fast_rcnn_inference([b], [s], [(10, 10)], 0.0, 0.5, 100),
                 lambda: D.select_detections([b], [s], [(10, 10)], 0.0, 0.5, 100),
                 lambda: D.paste_masks(torch.zeros((5, 1, 28, 28)), b, None, 20, 20),
                 lambda: D.coco_records([{"pred_boxes": b, "scores": s[:, 0], "pred_classes": torch.zeros(5, dtype=torch.int64)}], None,
                                        [(10, 10)], [(20, 20)], [1])):
        with pytest.raises(RuntimeError, match="no CPU fallback.*det_post_common"):
            call()
    sel = (
        (lambda: D.fast_rcnn_inference([], [], [], 0.0, 0.5, 100), "at least one image"),
        (lambda: D.fast_rcnn_inference([b], [s, s], [(10, 10)], 0.0, 0.5, 100), "per image"),
        (lambda: D.fast_rcnn_inference([b.double()], [s], [(10, 10)], 0.0, 0.5, 100), "float32 matrix"),
        (lambda: D.fast_rcnn_inference([b], [s[:, :1]], [(10, 10)], 0.0, 0.5, 100), "columns"),
        (lambda: D.fast_rcnn_inference([torch.zeros((5, 8))], [s], [(10, 10)], 0.0, 0.5, 100), "columns"),
        (lambda: D.fast_rcnn_inference([b[:4]], [s], [(10, 10)], 0.0, 0.5, 100), "rows of boxes"),
        (lambda: D.fast_rcnn_inference([b], [s], [(10,)], 0.0, 0.5, 100), r"\(h, w\)"),
        (lambda: D.fast_rcnn_inference([b], [s], [(10, float("inf"))], 0.0, 0.5, 100), "finite"),
        (lambda: D.fast_rcnn_inference([b], [s], [(10, 10)], float("nan"), 0.5, 100), "NaN"),
        (lambda: D.fast_rcnn_inference([b], [s], [(10, 10)], 0.0, "x", 100), "must be a number"),
        (lambda: D.fast_rcnn_inference([b], [s], [(10, 10)], 0.0, 0.5, 1.5), "integer"),
        (lambda: D.fast_rcnn_inference([torch.zeros((8193, 4))], [torch.zeros((8193, 2))], [(10, 10)], 0.0, 0.5, 100), "at most 8192"),
        (lambda: D.fast_rcnn_inference([torch.zeros((2731, 12))], [torch.zeros((2731, 4))], [(10, 10)], 0.0, 0.5, 100), "at most 8192"),
    )
    lg = torch.zeros((5, 1, 28, 28))
    cls = torch.zeros(5, dtype=torch.int64)
    det = {"pred_boxes": b, "scores": s[:, 0], "pred_classes": cls}
    paste = (
        (lambda: D.paste_masks(lg.double(), b, None, 20, 20), "float32 or bfloat16"),
        (lambda: D.paste_masks(lg[:4], b, None, 20, 20), "4 masks for 5 boxes"),
        (lambda: D.paste_masks(torch.zeros((5, 1, 28, 27)), b, None, 20, 20), "M, M"),
        (lambda: D.paste_masks(torch.zeros((5, 1, 129, 129)), b, None, 20, 20), "M <= 128"),
        (lambda: D.paste_masks(torch.zeros((5, 3, 28, 28)), b, None, 20, 20), "need pred_classes"),
        (lambda: D.paste_masks(lg, b, cls.int(), 20, 20), "int64"),
        (lambda: D.paste_masks(lg, b[:, :3], None, 20, 20), r"float32 \[n, 4\]"),
        (lambda: D.paste_masks(lg, b, None, 0, 20), "positive integers"),
        (lambda: D.paste_masks(lg, b, None, 1 << 16, 1 << 16), "2\\^31"),
        (lambda: D.paste_masks(lg, b, None, 20, 20, threshold=0.3), r"\[0.5, 1\]"),
        (lambda: D.paste_masks(lg, b, None, 20, 20, threshold=-1), r"\[0.5, 1\]"),
        (lambda: D.coco_records([det], None, [(10, 10)], [(20, 20)], [1, 2]), "per image"),
        (lambda: D.coco_records([det], None, [(0, 10)], [(20, 20)], [1]), "positive and finite"),
        (lambda: D.coco_records([det], None, [(10, 10)], [(20.5, 20)], [1]), "positive integers"),
        (lambda: D.coco_records([det], lg[:3], [(10, 10)], [(20, 20)], [1]), "3 masks for 5 boxes"),
        (lambda: D.coco_records([{"pred_boxes": b, "scores": s, "pred_classes": cls}], None, [(10, 10)], [(20, 20)], [1]), "scores float32"),
        (lambda: D.coco_records([{"pred_boxes": b, "scores": s[:, 0]}], None, [(10, 10)], [(20, 20)], [1]), "pred_classes"),
    )
    for call, what in sel + paste:
        with pytest.raises(ValueError, match=what):
            call()
    with pytest.raises(ValueError, match="same device"):
        D.fast_rcnn_inference([b], [s.to("meta")], [(10, 10)], 0.0, 0.5, 100)


def test_selection_restatement_on_the_constructed_blocks():
    """tests/nms_cases.py through select_numpy: the chains keep [A, C], 64 duplicates leave one, two zero-area boxes stay; a top-k cut is
    a prefix; the same box is kept once per class"""
    import nms_cases as NC
    boxes, kept = NC.constructed_boxes()
    b, s, shape = C.ranked_image(boxes)
    rows = C.select_numpy(b, s, shape, 0.05, NC.THRESH, -1)[3]
    NC.check_expected(rows)
    assert C.select_numpy(b, s, shape, 0.05, NC.THRESH, 65)[3].tolist() == kept[:65]
    ch = list(NC.CHAIN_IN_ONE_BLOCK)
    assert C.select_numpy(*C.ranked_image(boxes[ch]), 0.05, NC.THRESH, -1)[3].tolist() == [0, 2]
    assert C.select_numpy(*C.ranked_image(boxes[list(NC.DUPLICATES)]), 0.05, NC.THRESH, -1)[3].tolist() == [0]
    assert C.select_numpy(*C.ranked_image(boxes[list(NC.ZERO_AREA)]), 0.05, NC.THRESH, -1)[3].tolist() == [0, 1]
    for specific in (False, True):
        for (b, s, shape), want in zip(C.class_pairs(specific), C.CLASS_PAIRS_KEPT):
            got = C.select_numpy(b, s, shape, 0.05, NC.THRESH, -1)
            assert list(zip(got[3].tolist(), got[2].tolist())) == want
