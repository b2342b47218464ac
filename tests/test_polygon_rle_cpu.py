"""Polygon segmentations -> run-length records without a GPU: the sequential restatement of pycocotools' annToRLE for polygons
(unmore_amd.rle.polygon_crossings_numpy / from_polygons_numpy, what the device is compared against) pinned on cases worked out by
hand, its agreement with the C form of rleFrPoly's tail and with rleMerge (tests/polygon_rle_common.py), the restrictions, the
exports, and the evaluator's `polygons` switch up to the first launch."""
import math
import os
import re

import numpy as np
import pytest

from unmore_amd import _lib, coco_eval, rle
from coco_eval_common import dataset, dt_ann, gt_ann, rect
from polygon_rle_common import counts_of, fr_poly_counts_c, parity_mask, random_polygon, rle_merge_union, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("umr_poly_rle_workspace", "umr_poly_rle")


def _one(xy, h, w):
    return rle.from_polygons_numpy([[xy]], (h, w))[0]


def test_rectangle_by_hand():
    """vertices (2,1) (6,1) (6,4) (2,4): column x is inside from the line x = 2 up to the line x = 6, i.e. columns 2..5; row y from
    the line y = 1 up to y = 4, i.e. rows 1..3"""
    m = rle.polygon_mask_numpy([2, 1, 6, 1, 6, 4, 2, 4], 8, 10)
    want = np.zeros((8, 10), np.uint8)
    want[1:4, 2:6] = 1
    assert (m == want).all() and int(m.sum()) == 12
    rec = _one([2, 1, 6, 1, 6, 4, 2, 4], 8, 10)
    assert rec["size"] == [8, 10] and (rle.decode_numpy(rec) == want).all()
    assert counts_of(rec) == [17, 3, 5, 3, 5, 3, 5, 3, 36]


def test_triangle_and_ellipse_pins():
    assert int(rle.polygon_mask_numpy([10.5, 3.2, 40.1, 8.7, 22.3, 37.9], 48, 64).sum()) == 479
    t = np.arange(60) * 2 * np.pi / 60
    xy = np.stack([320 + 200 * np.cos(t) + 5 * np.sin(7 * t), 240 + 150 * np.sin(t)], axis=1).reshape(-1).tolist()
    u, v = rle.polygon_points_numpy(xy)
    assert len(u) == len(v) == 5066
    assert len(rle.polygon_crossings_numpy(xy, 480, 640)) == 808
    assert int(rle.polygon_mask_numpy(xy, 480, 640).sum()) == 94088
    assert rle.area(_one(xy, 480, 640)) == 94088


def test_closing_vertex_outside_and_clipping():
    tri = [10.5, 3.2, 40.1, 8.7, 22.3, 37.9]
    assert _one(tri + tri[:2], 48, 64) == _one(tri, 48, 64)                  # the ring is closed anyway: a zero-length edge adds nothing
    for outside in ([70.0, 5.0, 90.0, 5.0, 80.0, 30.0], [-30.0, -30.0, -5.0, -30.0, -5.0, -4.0], [5.0, 60.0, 30.0, 60.0, 20.0, 90.0]):
        assert counts_of(_one(outside, 48, 64)) == [48 * 64]
    # a vertex at negative coordinates clips: the square (-3,-3)..(4,4) leaves rows 0..3 of columns 0..3
    m = rle.polygon_mask_numpy([-3, -3, 4, -3, 4, 4, -3, 4], 6, 7)
    want = np.zeros((6, 7), np.uint8)
    want[0:4, 0:4] = 1
    assert (m == want).all()
    assert counts_of(_one([-3, -3, 4, -3, 4, 4, -3, 4], 6, 7)) == [0, 4, 2, 4, 2, 4, 2, 4, 20]
    # one and two vertices enclose nothing
    assert counts_of(_one([3.0, 3.0], 6, 7)) == [42] and counts_of(_one([1.0, 1.0, 5.0, 4.0], 6, 7)) == [42]


def test_a_crossing_at_the_end_of_the_image_gives_no_empty_last_run():
    """a square that reaches below the last row of the last column: its closing crossing is a = H*W"""
    sq = [3, 2, 9, 2, 9, 9, 3, 9]
    a = rle.polygon_crossings_numpy(sq, 6, 7)
    assert int(a.max()) == 6 * 7
    c = counts_of(_one(sq, 6, 7))
    assert c[-1] > 0 and sum(c) == 42 and c == fr_poly_counts_c(sq, 6, 7)
    want = np.zeros((6, 7), np.uint8)
    want[2:6, 3:7] = 1
    assert (rle.decode_numpy(_one(sq, 6, 7)) == want).all()


def test_union_is_or_not_the_parity_of_everything():
    tri = [10.5, 3.2, 40.1, 8.7, 22.3, 37.9]
    once, twice = rle.from_polygons_numpy([[tri], [tri, tri]], (48, 64))
    assert once == twice and rle.area(once) == 479
    other = [20.0, 5.0, 60.0, 5.0, 60.0, 30.0, 20.0, 30.0]
    both = rle.from_polygons_numpy([[tri, other]], (48, 64))[0]
    assert (rle.decode_numpy(both) == (parity_mask([tri], 48, 64) | parity_mask([other], 48, 64))).all()
    assert rle.area(both) > max(479, rle.area(_one(other, 48, 64)))          # overlapping: XOR would have cut the overlap out


def test_three_forms_agree_on_seeded_polygons():
    """per polygon: the C form (sort, differences, folded zeros) == the counts of the parity mask == the record's counts, with no
    interior zero; per annotation: rleMerge of the polygons' counts == the canonical counts of the OR.  Also the host's bound
    of a polygon's crossings, which sizes the device's lists, holds."""
    rng = np.random.default_rng(20240517)
    sizes = [(1, 1), (1, 9), (9, 1), (7, 5), (24, 31), (40, 33)]
    n = 0
    for it in range(420):
        h, w = sizes[it % len(sizes)]
        seg = [random_polygon(rng, h, w, int(rng.integers(1, 9)), int(rng.integers(0, 3))) for _ in range(int(rng.integers(1, 5)))]
        per_poly = []
        for xy in seg:
            c = fr_poly_counts_c(xy, h, w)
            assert c == [int(v) for v in rle.mask_to_counts(rle.polygon_mask_numpy(xy, h, w))], (it, xy)
            assert c == counts_of(_one(xy, h, w)) and all(v > 0 for v in c[1:]) and sum(c) == h * w
            per_poly.append(c)
            n += 1
        rec = rle.from_polygons_numpy([seg], (h, w))[0]
        assert rle_merge_union(per_poly, h, w) == counts_of(rec), (it, seg)
        assert rec == rle.encode_numpy(parity_mask(seg, h, w))
        polys, szs = rle._check_polygons([seg], (h, w), "test")
        cross_off = rle._poly_tables(polys, szs)[0][-8 * (len(seg) + 1):].view(np.int64)
        for q, xy in enumerate(seg):
            assert len(rle.polygon_crossings_numpy(xy, h, w)) <= cross_off[q + 1] - cross_off[q]
    assert n >= 1000


def test_sweep_polylines_land_on_and_beyond_the_sort_capacity():
    """the shapes the GPU test sorts in LDS and in memory: n edges over a w-wide image give n * w crossings"""
    cap = rle.POLY_SORT_LDS_KEYS
    assert cap == 4096 and len(rle.polygon_crossings_numpy(sweep(12, 256, 16), 12, 256)) == cap
    assert len(rle.polygon_crossings_numpy(sweep(12, 256, 18), 12, 256)) == cap + 512


def test_restrictions_raise_value_error():
    ok = [1.0, 1.0, 5.0, 1.0, 5.0, 5.0]
    for fn, kw in ((rle.from_polygons_numpy, {}), (rle.from_polygons, {"device": "cpu"})):        # before any launch: ValueError, not RuntimeError
        with pytest.raises(ValueError, match="coordinates"):
            fn([[ok + [2.0]]], (8, 8), **kw)
        with pytest.raises(ValueError, match="coordinates"):
            fn([[[]]], (8, 8), **kw)
        with pytest.raises(ValueError, match="not finite"):
            fn([[[1.0, math.nan, 5.0, 1.0, 5.0, 5.0]]], (8, 8), **kw)
        with pytest.raises(ValueError, match="not finite"):
            fn([[[1.0, math.inf, 5.0, 1.0, 5.0, 5.0]]], (8, 8), **kw)
        with pytest.raises(ValueError, match="2\\^20"):
            fn([[[1.0, 1.0, 2.0 ** 20 + 1, 1.0, 5.0, 5.0]]], (8, 8), **kw)
        with pytest.raises(ValueError, match="H\\*W < 2\\^31"):
            fn([[ok]], (1 << 16, 1 << 15), **kw)
        with pytest.raises(ValueError, match="sizes"):
            fn([[ok], [ok]], [(8, 8)], **kw)
        with pytest.raises(ValueError, match="not a polygon"):
            fn([{"size": [8, 8], "counts": "X1"}], (8, 8), **kw)
    assert len(rle._check_polygons([[[1.0, 1.0, 2.0 ** 20, -2.0 ** 20, 5.0, 5.0]]], (8, 8), "test")[0][0][0]) == 6      # the limit itself is accepted
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rle.from_polygons([[ok]], (8, 8), device="cpu")
    assert rle.from_polygons([], (8, 8), device="cuda") == [] and rle.from_polygons_numpy([], (8, 8)) == []
    for call in (lambda: rle.decode([[ok]], device="cpu"), lambda: rle.as_record([ok])):        # the decoders keep refusing polygons
        with pytest.raises(ValueError, match="polygon"):
            call()


def test_exports_are_declared_bound_and_resolvable():
    with open(os.path.join(ROOT, "include", "umr.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None
    ws = lib.umr_poly_rle_workspace
    assert ws.restype is not None and ws(-1, 1, 1, 1) == -1 and ws(1, -1, 1, 1) == -1 and ws(1, 1, -1, 1) == -1 and ws(1, 1, 1, -1) == -1
    # integer vertices + edge tables + counts + candidate counts + two crossing lists
    assert ws(10, 3, 2, 100) >= 10 * 8 + 13 * 8 + 3 * 4 + 2 * 8 + 2 * 100 * 4
    assert ws(10, 3, 2, 102) - ws(10, 3, 2, 100) == 16 and ws(1 << 32, 1, 1, 1 << 32) > 1 << 36
    assert lib.umr_poly_rle(None, None, None, None, None, 0, 0, 0, 0, 7, None, None, None, 0, None, 0, None) == -1
    assert b"poly_rle" in lib.umr_last_error_string()


def _polygon_gt():
    m = rect(12, 12, 2, 2, 4, 4)
    return m, dataset([(1, 12, 12)], [dict(gt_ann(7, 1, m), segmentation=[[2.0, 2.0, 6.0, 2.0, 6.0, 6.0, 2.0, 6.0]])])


def test_evaluator_polygons_switch_without_a_gpu():
    m, gt = _polygon_gt()
    ev = coco_eval.COCOEvaluator(gt, device="cpu")                            # the default keeps raising on the polygon
    ev.process(1, [dt_ann(1, m, 0.5)])
    with pytest.raises(ValueError, match="annotation 7.*polygon"):
        ev.evaluate()
    with pytest.raises(ValueError, match="polygons="):
        coco_eval.COCOEvaluator(gt, polygons="rasterise", device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # the conversion is a device call, made at construction
        coco_eval.COCOEvaluator(gt, polygons="rasterize", device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coco_eval.convert_polygons(gt, device="cpu")
    plain = dataset([(1, 12, 12)], [gt_ann(7, 1, m)])                         # nothing to convert: nothing is launched
    assert coco_eval.COCOEvaluator(plain, polygons="rasterize", device="cpu").gt["annotations"] == plain["annotations"]
    assert coco_eval.convert_polygons(plain, device="cpu") == plain
    lost = dataset([(1, 12, 12)], [dict(gt["annotations"][0], image_id=9)])
    with pytest.raises(ValueError, match="image 9"):
        coco_eval.convert_polygons(lost, device="cpu")
    # the polygon of _polygon_gt is the rectangle m: what the device has to reproduce
    assert rle.from_polygons_numpy([gt["annotations"][0]["segmentation"]], (12, 12))[0] == rle.encode_numpy(m)
