"""The host form of unmore_amd.detector_input (tests/det_input_common.py) against the reference's fixture and against PIL itself, and the
module's host side (draws, tables, boxes, argument checks) against the host form.  Every comparison is for equality."""
import numpy as np
import pytest
import torch

import det_input_common as C
from unmore_amd import detector_input as D
from unmore_amd import rle


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


@pytest.fixture(scope="module")
def mapped(fx):
    """the restatement's training outputs for the fixture batch"""
    out = []
    for img, annos, iid, (_, nh, nw, f) in zip(fx["images"], fx["annotations"], fx["image_ids"], fx["draws"]):
        dec = [dict(a, segmentation=rle.decode_numpy(a["segmentation"])) for a in annos]
        out.append(C.map_reference(img, dec, (nh, nw, f), image_id=iid))
    return out


def test_restatement_equals_the_reference_fixture(fx, mapped):
    """images, masks, boxes (as float32 bits), scores, classes, source, keep flags, height / width / is_single_object of every image; the
    fixture reaches flip and no flip, up- and down-scale, the max_size branch, no annotations, iscrowd, a vanishing mask, a degenerate
    box, an image that loses everything, scores present and absent"""
    flips = [d[3] for d in fx["draws"]]
    assert 0 < sum(flips) < len(flips)
    assert any(d[1] > im.shape[0] for d, im in zip(fx["draws"], fx["images"])) and any(d[1] < im.shape[0] for d, im in zip(fx["draws"], fx["images"]))
    assert any(C.output_shape(*im.shape[:2], d[0], 10 ** 9) != d[1:3] for d, im in zip(fx["draws"], fx["images"]))      # the max_size branch
    kinds = {"empty": 0, "all_dropped": 0, "some_dropped": 0, "crowd": 0}
    for k, (got, want, annos) in enumerate(zip(mapped, fx["expected"], fx["annotations"])):
        assert np.array_equal(got["image"], want["image"]), k
        assert np.array_equal(got["masks"], want["masks"]) and got["masks"].dtype == want["masks"].dtype, k
        assert got["boxes"].dtype == np.float32 and want["boxes"].dtype == np.float32
        assert np.array_equal(got["boxes"].view(np.uint32), want["boxes"].view(np.uint32)), k
        assert np.array_equal(got["scores"].view(np.uint32), want["scores"].view(np.uint32)), k
        assert np.array_equal(got["classes"], want["classes"]) and np.array_equal(got["source"], want["source"]), k
        assert np.array_equal(got["keep"], want["keep"]), k
        assert (got["height"], got["width"], got["is_single_object"]) == (want["height"], want["width"], want["is_single_object"]), k
        kinds["empty"] += len(annos) == 0
        kinds["all_dropped"] += len(annos) > 0 and not want["keep"].any()
        kinds["some_dropped"] += bool(want["keep"].any() and not want["keep"].all())
        kinds["crowd"] += any(a["iscrowd"] for a in annos)
    assert all(kinds.values()), kinds
    assert any("score" in a for annos in fx["annotations"] for a in annos) and any("score" not in a for annos in fx["annotations"] for a in annos)


def test_restatement_equals_the_fixture_at_test_time(fx):
    for k, (img, (_, nh, nw, f), want) in enumerate(zip(fx["images"], fx["test_draws"], fx["expected_test"])):
        got = C.map_reference(img, [], (nh, nw, f), is_train=False)
        assert f == 0 and np.array_equal(got["image"], want["image"]), k
        assert (got["height"], got["width"]) == (want["height"], want["width"]) == img.shape[:2], k


def test_restatement_equals_the_fixture_batch(fx):
    cfg = fx["cfg"]
    got, sizes = C.normalize_pad([e["image"] for e in fx["expected"]], cfg["pixel_mean"], cfg["pixel_std"], cfg["size_divisibility"])
    assert got.dtype == fx["batch"].dtype == np.float32 and got.shape == fx["batch"].shape
    assert np.array_equal(got.view(np.uint32), fx["batch"].view(np.uint32))
    assert sizes == fx["image_sizes"]


def test_draw_transforms_reproduces_the_fixture_draws(fx):
    cfg = fx["cfg"]
    sizes = [im.shape[:2] for im in fx["images"]]
    got = D.draw_transforms(sizes, min_size=cfg["min_size"], max_size=cfg["max_size"], np_random=np.random.RandomState(cfg["seed"]))
    assert got == [d[1:] for d in fx["draws"]]
    np.random.seed(cfg["seed"])                                      # the default stream is the global one, as in the reference
    assert D.draw_transforms(sizes, min_size=cfg["min_size"], max_size=cfg["max_size"]) == got
    test = D.draw_transforms(sizes, min_size=cfg["min_size_test"], max_size=cfg["max_size_test"], is_train=False,
                             np_random=np.random.RandomState(cfg["seed"] + 1))
    assert test == [d[1:] for d in fx["test_draws"]]
    # the other sampling style, the other flip, no resize: against the host form on equally seeded streams
    for style, ms, flip in (("range", (20, 70), "vertical"), ("choice", (0, 33), "horizontal"), ("choice", 48, "none")):
        got = D.draw_transforms(sizes, min_size=ms, max_size=90, sample_style=style, flip=flip, np_random=np.random.RandomState(5))
        ms2 = (ms, ms) if isinstance(ms, int) else ms
        assert got == [d[1:] for d in C.draw(sizes, ms2, 90, style, flip, True, np.random.RandomState(5))], style
    assert any(t[:2] == s for t, s in zip(D.draw_transforms(sizes, min_size=(0, 0), np_random=np.random.RandomState(1)), sizes))


def test_module_tables_equal_the_host_form():
    pairs = {(h, nh) for h, w, nh, nw, _ in C.resize_cases()} | {(w, nw) for h, w, nh, nw, _ in C.resize_cases()}
    pairs |= {(480, 240), (375, 800), (640, 1535), (4000, 240), (1024, 1024)}
    for inn, out in sorted(pairs):
        lo, n, k = D.bilinear_table(inn, out)
        if inn == out:                                               # PIL skips the pass; the table returns the byte itself
            assert lo.tolist() == list(range(out)) and (n == 1).all() and (k == 1 << 22).all() and k.shape == (out, 1)
        else:
            lo2, n2, k2 = C.axis_table(inn, out)
            assert np.array_equal(lo, lo2) and np.array_equal(n, n2) and np.array_equal(k, k2), (inn, out)
            assert (k >= 0).all() and abs(int(k.sum(1).max()) - (1 << 22)) <= k.shape[1] and (lo + n <= inn).all() and (n >= 1).all()
        assert np.array_equal(D.nearest_table(inn, out), C.nearest_table(inn, out)), (inn, out)


def test_tile_shapes_fit_the_lds_budget_and_reach_every_form():
    forms = set()
    cases = [(h, nh) for h, w, nh, nw, _ in C.resize_cases()] + [(4000, 240), (480, 1024), (12000, 2)]
    for H, nh in cases:
        lo, n, _ = D.bilinear_table(H, nh)
        th, tw = D.tile_shape(lo, n, nh)
        y0 = np.arange(0, nh, th)
        y1 = np.minimum(y0 + th, nh) - 1
        assert int((lo[y1] + n[y1] - lo[y0]).max()) * tw <= D.LDS_PIX and 1 <= tw <= D.MAX_TW and th in D.TILE_ROWS, (H, nh)
        assert th == 1 or tw == D.MAX_TW
        forms.add("full" if th == 32 else "rows" if tw == D.MAX_TW else "columns")
    assert forms == {"full", "rows", "columns"}
    # a 4000-pixel ImageNet side down to 240, 35-tap rows: 8 output rows read 7 * 16.7 + 35 = 152 input rows (x 64 columns fit), 16 would read 285
    assert D.tile_shape(*D.bilinear_table(4000, 240)[:2], 240) == (8, 64)
    # the device test's batch: 400 -> 40 rows reads 15 * 10 + 21 = 171 > 170 input rows for 32 output rows at 64 columns, 16 rows fit; one
    # output row of 700 -> 4 reads 351 input rows, which fit at 16 columns (5616 staged pixels) and not at 32 (11232 > 10880)
    want = {(400, 40): (16, 64), (700, 4): (1, 16)}
    for c in C.resize_cases():
        assert D.tile_shape(*D.bilinear_table(c[0], c[2])[:2], c[2]) == want.get((c[0], c[2]), (32, 64)), c
    with pytest.raises(ValueError, match="input rows"):
        D.tile_shape(*D.bilinear_table(30000, 1)[:2], 1)


def test_boxes_equal_the_host_form(fx):
    rng = np.random.RandomState(3)
    for H, W, nh, nw, f in C.resize_cases()[::5]:
        b = rng.uniform(-3, max(H, W) + 3, (7, 4))
        assert np.array_equal(D.transform_boxes(b, H, W, nh, nw, f).view(np.uint32), C.transform_boxes(b, H, W, nh, nw, f).view(np.uint32))
    for annos in fx["annotations"]:
        for a in annos:
            assert np.array_equal(D.convert_box(a["bbox"], a["bbox_mode"]), C.convert_box(a["bbox"], a["bbox_mode"]))
    # a list goes through float32 (Detectron2's torch.tensor(box)), an array and an XYXY box do not
    assert D.convert_box([0.1, 0.2, 0.3, 0.4], D.XYWH_ABS)[2] == float(np.float32(0.1) + np.float32(0.3))
    assert D.convert_box(np.array([0.1, 0.2, 0.3, 0.4]), D.XYWH_ABS)[2] == 0.1 + 0.3
    assert D.convert_box([0.1, 0.2, 0.3, 0.4], D.XYXY_ABS).tolist() == [0.1, 0.2, 0.3, 0.4]
    assert D.convert_box([1, 2, 3, 4], D.XYWH_ABS).tolist() == [1.0, 2.0, 4.0, 6.0]


def test_restatement_equals_pil():
    """the size list of the device test and three full-scale pairs, bilinear on RGB and nearest on L, byte for byte"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(0)
    cases = [c[:4] for c in C.resize_cases()] + [(a[0], a[1], b[0], b[1]) for a, b in C.FULL_SCALE]
    for H, W, nh, nw in cases:
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        assert np.array_equal(C.resize_bilinear(img, nh, nw), np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))), (H, W, nh, nw)
        m = (rng.rand(H, W) < 0.3).astype(np.uint8)
        assert np.array_equal(C.resize_nearest(m, nh, nw), np.asarray(Image.fromarray(m).resize((nw, nh), Image.NEAREST))), (H, W, nh, nw)


def test_nearest_table_is_repeated_addition():
    """Search the size pairs (side <= 2048) for the first one where the repeated-addition table and the (i + 0.5) * a table differ: it is
    the pair the device test uses (C.NEAREST_PAIR), and PIL sides with the addition."""
    found = None
    for out in range(1, 2049):
        for inn in range(1, 2049):
            a = inn / out
            steps = np.full(out, a)
            steps[0] = 0.5 * a
            if not np.array_equal(np.add.accumulate(steps).astype(np.int64), ((np.arange(out) + 0.5) * a).astype(np.int64)):
                found = (inn, out)
                break
        if found:
            break
    assert found == C.NEAREST_PAIR
    inn, out = found
    add, mul = C.nearest_table(inn, out), C.nearest_table_mul(inn, out)
    assert not np.array_equal(add, mul) and add.max() < inn
    m = np.stack([np.arange(inn) % 2, np.arange(inn) % 3 == 0]).astype(np.uint8)        # two rows
    assert not np.array_equal(C.resize_nearest(m, 2, out), m[:, mul])
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.fromarray(m).resize((out, 2), Image.NEAREST)), C.resize_nearest(m, 2, out))


def test_argument_errors_are_value_errors_before_anything_runs():
    img = torch.zeros((8, 9, 3), dtype=torch.uint8)
    ann = {"bbox": [1.0, 1.0, 3.0, 3.0], "bbox_mode": D.XYWH_ABS, "segmentation": torch.ones((8, 9), dtype=torch.bool)}
    t = [(8, 9, 0)]
    bad_calls = [
        ("images\\[0\\]", lambda: D.map_batch([img.float()], [[ann]], t)),
        ("images\\[0\\]", lambda: D.map_batch([img.permute(2, 0, 1)], [[ann]], t)),
        ("images\\[0\\]", lambda: D.resize_images([torch.zeros((0, 9, 3), dtype=torch.uint8)], [(4, 4)], [0])),
        ("transforms\\[0\\]", lambda: D.map_batch([img], [[ann]], [(0, 9, 0)])),
        ("transforms\\[0\\]", lambda: D.resize_images([img], [(4, -1)], [0])),
        ("flip", lambda: D.resize_images([img], [(4, 4)], [3])),
        ("1 transforms for 2", lambda: D.map_batch([img, img], [[ann], [ann]], t)),
        ("annotation lists", lambda: D.map_batch([img], [], t)),
        ("annotations\\[0\\]\\[0\\].*size", lambda: D.map_batch([img], [[dict(ann, segmentation=torch.ones((9, 8), dtype=torch.bool))]], t)),
        ("annotations\\[0\\]\\[0\\].*size", lambda: D.map_batch([img], [[dict(ann, segmentation={"size": [9, 8], "counts": "X2"})]], t)),
        ("annotations\\[0\\]\\[0\\].*polygon", lambda: D.map_batch([img], [[dict(ann, segmentation=[[1, 1, 4, 1, 4, 4]])]], t)),
        ("annotations\\[0\\]\\[0\\].*keypoints", lambda: D.map_batch([img], [[dict(ann, keypoints=[1, 1, 2])]], t)),
        ("annotations\\[0\\]\\[0\\].*segmentation", lambda: D.map_batch([img], [[{k: v for k, v in ann.items() if k != "segmentation"}]], t)),
        ("annotations\\[0\\]\\[0\\].*segmentation", lambda: D.map_batch([img], [[dict(ann, segmentation=torch.ones((8, 9)))]], t)),
        ("annotations\\[0\\]\\[0\\].*bbox", lambda: D.map_batch([img], [[dict(ann, bbox=[1.0, 2.0, 3.0])]], t)),
        ("annotations\\[0\\]\\[0\\].*bbox_mode", lambda: D.map_batch([img], [[dict(ann, bbox_mode=4)]], t)),
        ("annotations\\[0\\].*score", lambda: D.map_batch([img], [[dict(ann, score=0.5), ann]], t)),
        ("annotations\\[0\\].*sem_seg", lambda: D.map_batch([img], [{"sem_seg": None}], t)),
        ("masks\\[0\\]", lambda: D.resize_masks([torch.zeros((2, 8, 9))], [(4, 4)], [0])),
        ("masks\\[0\\]", lambda: D.resize_masks([torch.zeros((8, 9), dtype=torch.bool)], [(4, 4)], [0])),
        ("2 flips", lambda: D.resize_masks([torch.zeros((1, 8, 9), dtype=torch.bool)], [(4, 4)], [0, 1])),
        ("images\\[0\\]", lambda: D.preprocess_image([img], [1., 2., 3.], [1., 1., 1.])),
        ("three values", lambda: D.preprocess_image([img.permute(2, 0, 1)], [1., 2.], [1., 1., 1.])),
        ("non-zero", lambda: D.preprocess_image([img.permute(2, 0, 1)], [1., 2., 3.], [1., 0., 1.])),
        ("size_divisibility", lambda: D.preprocess_image([img.permute(2, 0, 1)], [1., 2., 3.], [1., 1., 1.], -2)),
        ("sample_style", lambda: D.draw_transforms([(8, 9)], min_size=8, sample_style="uniform")),
        ("flip", lambda: D.draw_transforms([(8, 9)], min_size=8, flip="both")),
        ("two values", lambda: D.draw_transforms([(8, 9)], min_size=(8, 9, 10), sample_style="range")),
        ("not positive", lambda: D.draw_transforms([(0, 9)], min_size=8)),
    ]
    for pattern, call in bad_calls:
        with pytest.raises(ValueError, match=pattern):
            call()
