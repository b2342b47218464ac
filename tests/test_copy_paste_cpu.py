"""unmore_amd.copy_paste without a GPU: the torch restatement against the fixture the reference's own copy_and_paste wrote
(tests/golden/make_golden_copy_paste.py), the random draws, the documented float32 resize order against F.interpolate, and the
argument errors."""
import random

import numpy as np
import pytest
import torch

import torch.nn.functional as F

from copy_paste_common import blob_item, copy_paste_reference, interpolate_bytes, load_fixture, resize_bytes_f32, resize_mask_bits


def test_restatement_equals_the_reference_fixture():
    """Every branch of the fixture batch: masks, boxes, instance order, source and the unchanged items are exactly the reference's; so is
    the image (same F.interpolate on the same torch)."""
    items, params, expected, _, _ = load_fixture()
    got = copy_paste_reference(items[::-1], items, params)
    assert [e["unchanged"] for e in expected] == [g["unchanged"] for g in got]
    assert sum(e["unchanged"] for e in expected) >= 3 and sum(p is None for p in params) == 1
    for p, (g, e) in enumerate(zip(got, expected)):
        if e["unchanged"]:
            assert g["image"] is items[p]["image"] and g["masks"] is items[p]["masks"] and g["boxes"] is items[p]["boxes"], p
        assert np.array_equal(g["masks"].numpy(), e["masks"]), p
        assert np.array_equal(g["boxes"].numpy(), e["boxes"]), p
        assert np.array_equal(g["source"].numpy(), e["source"]), p
        assert np.array_equal(g["image"].numpy(), e["image"]), p
    # the branches the fixture was built for
    assert items[1]["masks"].shape[0] == 0 and not expected[1]["unchanged"]                           # empty unlabeled image
    assert (expected[8]["source"][:, 0] == 0).sum() == 1 and items[8]["masks"].shape[0] == 2          # an existing instance erased
    assert any(int(items[2]["masks"][j].sum()) == 0 for j in range(items[2]["masks"].shape[0]))       # an existing mask of area 0
    assert items[4]["image"].shape != items[3]["image"].shape


def test_draw_params_replays_the_reference_draws():
    from unmore_amd.copy_paste import draw_params
    items, params, _, seed, cfg = load_fixture()
    B = len(items)
    n_lab = [items[B - 1 - p]["masks"].shape[0] for p in range(B)]
    sizes = [tuple(it["image"].shape[1:]) for it in items]
    got = draw_params(n_lab, sizes, py_random=random.Random(seed), np_random=np.random.RandomState(seed), **cfg)
    # a literal replay of the six draws (train_loop.py:132-163)
    pr, nr = random.Random(seed), np.random.RandomState(seed)
    for p in range(B):
        n, (hu, wu) = n_lab[p], sizes[p]
        draw = pr.random()
        if cfg["rate"] >= draw and n > 0:
            num_copy = 1 if n == 1 else nr.randint(1, max(1, n))
            choice = nr.choice(n, num_copy, replace=False)
            ratio = pr.uniform(cfg["min_ratio"], cfg["max_ratio"])
            w_new, h_new = int(ratio * wu), int(ratio * hu)
            w_shift = pr.randint(0, wu - w_new)
            h_shift = pr.randint(0, hu - h_new)
            lit = (choice, ratio, h_new, w_new, h_shift, w_shift)
        else:
            lit = None
        for other in (lit, params[p]):
            if other is None:
                assert got[p] is None, p
            else:
                assert np.array_equal(got[p][0], other[0]) and tuple(got[p][1:]) == tuple(other[1:]), p
    # the global streams are the default; without random_num every instance is copied; rate 0 draws once per pair and copies nothing
    random.seed(3)
    np.random.seed(3)
    a = draw_params([3, 0, 2], [(20, 30)] * 3, 1.0, False, 0.3, 1.0)
    b = draw_params([3, 0, 2], [(20, 30)] * 3, 1.0, False, 0.3, 1.0, py_random=random.Random(3), np_random=np.random.RandomState(3))
    assert a[1] is None and b[1] is None and sorted(a[0][0].tolist()) == [0, 1, 2]
    assert all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for x, y in ((a[0], b[0]), (a[2], b[2])))
    pr = random.Random(5)
    assert draw_params([3, 2], [(20, 30)] * 2, 0.0, True, 0.3, 1.0, py_random=pr, np_random=np.random.RandomState(5)) == [None, None]
    q = random.Random(5)
    q.random(), q.random()
    assert pr.random() == q.random()


def test_resize_bytes_f32_against_interpolate():
    """The kernel's float32 operation order against F.interpolate(...).byte(): every byte within one level, at most 1 % different
    (measured 0.083 %, all by one level: see the print).  torch resizes a 3-channel image with another kernel -- another operation order,
    about 1 % of the bytes of these images one level off -- when it runs on ONE thread; the comparison is with the kernel the
    reference's training process runs, so the thread count is pinned to at least two for the duration of the test."""
    rng = np.random.RandomState(0)
    n_threads = torch.get_num_threads()
    torch.set_num_threads(max(2, n_threads))
    try:
        differ = total = worst = 0
        for case in range(40):
            H, W = (int(v) for v in rng.randint(5, 120, 2))
            h, w = (int(v) for v in rng.randint(1, 130, 2))
            if case == 0:
                h, w = H, W
            img = blob_item(rng, H, W, 0)["image"]
            ref = interpolate_bytes(img, h, w).numpy().astype(np.int64)
            got = resize_bytes_f32(img, h, w).astype(np.int64)
            d = np.abs(got - ref)
            differ, total, worst = differ + int((d > 0).sum()), total + d.size, max(worst, int(d.max()))
    finally:
        torch.set_num_threads(n_threads)
    print(f"resize_bytes_f32 vs F.interpolate: {differ} of {total} bytes differ ({100.0 * differ / total:.3f} %), worst {worst} level(s)")
    assert worst <= 1
    assert differ <= 0.01 * total


def test_mask_bit_rule_equals_interpolate_bool():
    """The kernel's mask rule -- any tap with a non-zero weight, source index in one fused rounding -- gives F.interpolate(...).bool()
    exactly: 60 seeded noise masks at random sizes, and the sizes at which a source index formed with two roundings lands on an
    integer that the fused one misses (19 -> 95: scale 0.2f, dst 2)."""
    rng = np.random.RandomState(3)
    cases = [(19, 19, 95, 95), (18, 47, 90, 75), (15, 82, 95, 24), (7, 5, 7, 5), (1, 1, 9, 3), (9, 3, 1, 1)]
    cases += [tuple(int(v) for v in np.concatenate([rng.randint(1, 90, 2), rng.randint(1, 100, 2)])) for _ in range(60)]
    for H, W, h, w in cases:
        m = torch.from_numpy(rng.rand(3, H, W) < 0.2)
        ref = F.interpolate(m[None].float(), size=(h, w), mode="bilinear", align_corners=False).bool()[0].numpy()
        assert np.array_equal(resize_mask_bits(m, h, w), ref), (H, W, h, w)


def _item(H, W, N, dev="cpu"):
    it = blob_item(np.random.RandomState(H + W + N), H, W, N)
    return {k: v.to(dev) for k, v in it.items()}


def test_argument_errors_before_any_launch():
    from unmore_amd.copy_paste import copy_and_paste
    lab, unl = _item(12, 16, 2), _item(10, 14, 1)
    ok = (np.array([1]), 0.5, 5, 7, 1, 2)
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        copy_and_paste([lab], [unl], [ok])
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        copy_and_paste([lab], [unl], [None])
    for bad, what in (((np.array([1]), 0.01, 0, 7, 1, 2), "zero-sized"), ((np.array([1]), 0.01, 5, 0, 1, 2), "zero-sized"),
                      ((np.array([2]), 0.5, 5, 7, 1, 2), "choice"), ((np.array([1, 1]), 0.5, 5, 7, 1, 2), "choice"),
                      ((np.array([], dtype=np.int64), 0.5, 5, 7, 1, 2), "choice"), ((np.array([1]), 0.5, 5, 7, 6, 2), "leaves"),
                      ((np.array([1]), 0.5, 5, 7, 1, 8), "leaves"), ((np.array([1]), 0.5, 5, 7, -1, 2), "leaves"), ((1, 2, 3), "params")):
        with pytest.raises(ValueError, match=what):
            copy_and_paste([lab], [unl], [bad])
    with pytest.raises(ValueError, match="without instances"):
        copy_and_paste([_item(12, 16, 0)], [unl], [ok])
    with pytest.raises(ValueError, match="2 params entries"):
        copy_and_paste([lab], [unl], [ok, None])
    with pytest.raises(ValueError, match="labeled items"):
        copy_and_paste([lab, lab], [unl], [ok])
    # H * W >= 2^24 (a view: nothing of that size is allocated)
    big = {"image": torch.zeros(1, 1, 1, dtype=torch.uint8).expand(3, 4096, 4096), "masks": torch.zeros(0, 4096, 4096, dtype=torch.bool),
           "boxes": torch.zeros(0, 4)}
    with pytest.raises(ValueError, match="2\\^24"):
        copy_and_paste([lab], [big], [(np.array([1]), 0.5, 2048, 2048, 0, 0)])
    # shapes and dtypes
    for key, val, what in (("image", lab["image"].float(), "image must be uint8"), ("image", lab["image"][:2], "image must be uint8"),
                           ("masks", lab["masks"][:, :-1], "masks must be"), ("masks", lab["masks"].float(), "masks must be"),
                           ("boxes", lab["boxes"].double(), "boxes must be"), ("boxes", lab["boxes"][:1], "boxes must be"),
                           ("boxes", None, "needs a tensor")):
        broken = dict(lab)
        broken[key] = val
        with pytest.raises(ValueError, match=what):
            copy_and_paste([broken], [unl], [ok])
        with pytest.raises(ValueError, match=what):
            copy_and_paste([unl], [broken], [None])
    assert copy_and_paste([], [], []) == []
