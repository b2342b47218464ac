"""The existence classifier's training item on the MI355X (synthesize_classifier_items, umr_bg_square,
umr_crop_resize_ragged) against the CPU restatement of datasets.py:285-349 (tests/clf_items_common.py): boxes, flags and
labels equal, images within the bilinear kernel's 2e-6, mask sums within 1e-3.
Measured on an MI355X: image error at most 1.2e-7, mask sums within 6e-8 relative; this file and test_clf_evaluate_gpu.py
together (9 tests) take 4.4 s."""
import random

import numpy as np
import pytest
import torch

import clf_items_common as C

pytestmark = pytest.mark.gpu

SIZES = [(375, 500), (500, 333), (96, 128), (33, 1)]
WIDE = (621, 2100)      # wider than 2048, and large enough for distances above 256 pixels (16.16 values above 2^24)


def _dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _image(rng, h, w):
    return torch.from_numpy(rng.random((3, h, w)).astype(np.float32))


def _ellipse(rng, h, w, value=255, lo=0.3, hi=0.7):
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(lo, hi) * h, rng.uniform(lo, hi) * w
    ry, rx = rng.uniform(h / 8 + 1, h / 3 + 1), rng.uniform(w / 8 + 1, w / 3 + 1)
    return torch.from_numpy(((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1) * value).astype(np.uint8))


def _bg_cases():
    """(name, full mask u8 [h,w]) for the background branch"""
    rng = np.random.default_rng(41)
    cases = [(f"ellipse {h}x{w}", _ellipse(rng, h, w)) for (h, w) in SIZES]
    cases.append(("two ellipses, raw values 1 and 200", torch.maximum(_ellipse(rng, 375, 500, 1), _ellipse(rng, 375, 500, 200))))
    cases.append(("no background", torch.full((96, 128), 255, dtype=torch.uint8)))
    m = torch.full((120, 90), 255, dtype=torch.uint8)
    m[:, 0] = 0
    cases.append(("background one pixel thin along the left edge", m))
    cases.append(("empty mask", torch.zeros((375, 500), dtype=torch.uint8)))
    m = torch.full((200, 333), 9, dtype=torch.uint8)
    for (y, x) in ((120, 250), (20, 200), (20, 30), (120, 100)):      # four equal 41 x 41 holes, not in raster order
        m[y:y + 41, x:x + 41] = 0
    cases.append(("several equal maxima", m))
    m = torch.zeros(WIDE, dtype=torch.uint8)
    m[300, 400] = 255
    m[17, 1900] = 3
    m[500:520, 1000:1010] = 128
    cases.append(("wide and large", m))
    return cases


def test_background_squares_equal_the_restatement():
    from unmore_amd.labels import background_squares
    cases = _bg_cases()
    want = []
    for name, m in cases:
        x1, y1, x2, y2 = C.bg_square(m.numpy(), 10)                     # the literal form: pad 10, transform, slice, argmax, int()
        h, w = m.shape
        assert 0 <= x1 <= w and 0 <= x2 <= w and 0 <= y1 <= h and 0 <= y2 <= h, name
        want.append([x1, y1, x2, y2, int(x2 > x1 and y2 > y1)])
    by_name = dict(zip((n for n, _ in cases), want))
    # the inputs are what they claim to be (checked on the CPU side, before the device is asked)
    assert by_name["no background"] == [0, 0, 0, 0, 0]
    assert by_name["background one pixel thin along the left edge"][4] == 0 and by_name[f"ellipse 33x1"][4] == 0
    assert by_name["empty mask"][4] == 1
    # the hole at (y 20, x 30), columns 30..70 and rows 20..60: centre (x 50, y 40), 21 pixels from the object, r = 21 * 0.955 = 20.055
    assert by_name["several equal maxima"] == [29, 19, 70, 60, 1]
    fixed = C.zero_border_fixed(cases[-1][1].numpy() == 0)
    # float32 no longer holds every 16.16 value there: the maximum itself (311 * 62587, odd) is not representable, so the
    # radius is the rounded value and neighbouring fixed-point values share a float32
    assert fixed.max() >= 1 << 24 and int(np.float32(fixed.max())) != int(fixed.max())
    got = background_squares([m.to(_dev()) for _, m in cases]).cpu().tolist()
    for (name, _), g, w in zip(cases, got, want):
        assert g == w, (name, g, w)


def _fg_items():
    """(image, top-1 mask, full mask, coin, params, what) -- the foreground branch and the fall-through into it"""
    rng = np.random.default_rng(43)
    items = []

    def add(h, w, top1, full, coin, params, what):
        items.append((_image(rng, h, w), top1, full if full is not None else top1.clone(), coin, params, what))

    add(375, 500, _ellipse(rng, 375, 500), None, False, (40, 60, 300, 280), "0/255 mask, clear positive")
    m = torch.zeros((500, 333), dtype=torch.uint8)
    m[20:80, 30:90] = 255
    add(500, 333, m, None, False, (250, 150, 200, 160), "0/255 mask, the crop misses the object: sum 0")
    m = torch.zeros((375, 500), dtype=torch.uint8)
    m[100:260, 150:350] = 1
    add(375, 500, m, None, False, (50, 100, 300, 300), "0/1-valued PNG, large object: sum = pixels / 255 above 1")
    m = torch.zeros((375, 500), dtype=torch.uint8)
    m[100:120, 150:170] = 1
    add(375, 500, m, None, False, (50, 100, 300, 300), "0/1-valued PNG, small object: sum = pixels / 255 below 1")
    add(96, 128, _ellipse(rng, 96, 128), torch.full((96, 128), 255, dtype=torch.uint8), True, (10, 20, 60, 70),
        "coin says background, the full mask has none: falls through")
    add(33, 1, torch.full((33, 1), 255, dtype=torch.uint8), torch.zeros((33, 1), dtype=torch.uint8), True, (3, 0, 20, 1),
        "one column: the square is empty, falls through")
    add(40, 2100, _ellipse(rng, 40, 2100), None, False, (5, 700, 30, 1200), "wider than 2048")
    add(96, 128, _ellipse(rng, 96, 128), None, False, (0, 0, 96, 128), "whole image")
    return items


def _bg_items():
    rng = np.random.default_rng(47)
    items = []
    for (h, w) in SIZES[:3] + [(40, 2100)]:
        full = _ellipse(rng, h, w)
        items.append((_image(rng, h, w), full.clone(), full, True, None, f"background square {h}x{w}"))
    items.append((_image(rng, 375, 500), torch.zeros((375, 500), dtype=torch.uint8), torch.zeros((375, 500), dtype=torch.uint8), True, None,
                  "empty masks: the square is the image's largest"))
    return items


@pytest.mark.parametrize("S", [128, 50])
def test_items_of_both_branches_equal_the_restatement(S):
    from unmore_amd import synthesize_classifier_items
    dev = _dev()
    fg, bg = _fg_items(), _bg_items()
    items = [fg[0], bg[0], fg[1], bg[1], fg[2], fg[3], bg[2], fg[4], fg[5], bg[3], fg[6], bg[4], fg[7]]
    want = [C.classifier_item(im, m1, mf, coin, p, S) for (im, m1, mf, coin, p, _) in items]
    # the label is a threshold on a float sum: every item's float64 sum stays clear of it, and the set covers both sides
    sums = [info["mask_sum"] for (_, _, info) in want]
    assert all(abs(s - 1.0) >= 1e-2 for s in sums), sums
    names = [it[5] for it in items]
    by = dict(zip(names, want))
    assert by["0/255 mask, the crop misses the object: sum 0"][2]["mask_sum"] == 0.0
    assert by["0/255 mask, clear positive"][2]["mask_sum"] > 100
    assert 1.01 < by["0/1-valued PNG, large object: sum = pixels / 255 above 1"][2]["mask_sum"] < 100
    assert 0 < by["0/1-valued PNG, small object: sum = pixels / 255 below 1"][2]["mask_sum"] < 0.99
    assert [info["branch"] for (_, _, info) in want] == [1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 1]
    out, labels, info = synthesize_classifier_items([it[0].to(dev) for it in items], [it[1].to(dev) for it in items],
                                                    [it[2].to(dev) for it in items], S, coins=[it[3] for it in items],
                                                    params=[it[4] for it in items])
    B = len(items)
    assert out.shape == (B, 3, S, S) and out.dtype == torch.float32 and labels.shape == (B, 1) and labels.dtype == torch.float32
    assert info["branch"].cpu().tolist() == [w[2]["branch"] for w in want]
    assert info["boxes"].cpu().tolist() == [list(w[2]["box"]) for w in want]
    assert labels.cpu().view(-1).tolist() == [w[1] for w in want]
    got_sums = info["mask_sum"].cpu().tolist()
    for name, g, s in zip(names, got_sums, sums):
        print(f"{name}: mask_sum {g!r} (float64 restatement {s!r})")
        assert abs(g - s) <= 1e-3 * (abs(s) if abs(s) >= 1 else 1.0), (name, g, s)
    for b, name in enumerate(names):
        err = (out[b].cpu() - want[b][0]).abs().max().item()
        print(f"{name}: image max abs error {err:.3e}")
        torch.testing.assert_close(out[b].cpu(), want[b][0], atol=2e-6, rtol=0, msg=lambda m, n=name: f"{n}: {m}")


def test_mask_sum_is_reproducible_across_calls_and_batch_compositions():
    """The per-item mask sum decides a label: it is bit-identical across calls and across batch compositions (one workgroup per
    item and plane, fixed order of additions: no dependence on the grid)."""
    from unmore_amd import synthesize_classifier_items
    dev = _dev()
    fg = _fg_items()[:4]
    args = lambda its: ([it[0].to(dev) for it in its], [it[1].to(dev) for it in its], [it[2].to(dev) for it in its], 64)   # noqa: E731
    _, _, a = synthesize_classifier_items(*args(fg), coins=[False] * 4, params=[it[4] for it in fg])
    _, _, b = synthesize_classifier_items(*args(fg), coins=[False] * 4, params=[it[4] for it in fg])
    rev = fg[::-1] + fg[:2]
    _, _, c = synthesize_classifier_items(*args(rev), coins=[False] * 6, params=[it[4] for it in rev])
    assert torch.equal(a["mask_sum"], b["mask_sum"])
    assert torch.equal(c["mask_sum"][:4].flip(0), a["mask_sum"]) and torch.equal(c["mask_sum"][4:], a["mask_sum"][:2])


def test_draws_follow_the_reference_order():
    """coins=None, params=None: coins come from Python's `random` in item order, crop boxes from torch's CPU generator for
    exactly the foreground items, in item order; items that succeed on the background branch consume no torch draws."""
    from unmore_amd import synthesize_classifier_items
    from unmore_amd.labels import random_resized_crop_params
    dev = _dev()
    rng = np.random.default_rng(53)
    sizes = [(96, 128), (120, 90), (64, 64), (33, 1), (100, 150), (375, 500), (80, 80), (128, 96)]
    images = [_image(rng, h, w) for (h, w) in sizes]
    top1 = [_ellipse(rng, h, w) for (h, w) in sizes]
    full = [m.clone() for m in top1]
    full[2] = torch.full(sizes[2], 255, dtype=torch.uint8)                  # no background: a True coin falls through
    random.seed(3)
    coins = [random.random() < 0.5 for _ in sizes]
    assert coins == [True, False, True, False, False, True, True, False]    # item 2 falls through, items 0, 5, 6 stay background
    expect_branch = [0, 1, 1, 1, 1, 0, 0, 1]
    assert [int(not (c and C.bg_square_zero_border(f.numpy())[4])) for c, f in zip(coins, full)] == expect_branch
    g = torch.Generator()
    runs = []
    for _ in range(2):
        random.seed(3)
        g.manual_seed(7)
        out, labels, info = synthesize_classifier_items([t.to(dev) for t in images], [t.to(dev) for t in top1], [t.to(dev) for t in full], 64,
                                                        generator=g)
        runs.append((out.cpu(), labels.cpu(), {k: v.cpu() for k, v in info.items()}, g.get_state().clone(), random.getstate()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    assert runs[0][2]["branch"].tolist() == expect_branch
    # replay the draws on the host: the same boxes, and the generator ends in the same state (nothing else was drawn)
    g.manual_seed(7)
    for b, (h, w) in enumerate(sizes):
        if expect_branch[b]:
            t, l, ch, cw = random_resized_crop_params(h, w, ratio=(3.0 / 4.0, 4.0 / 3.0), generator=g)
            assert runs[0][2]["boxes"][b].tolist() == [l, t, l + cw, t + ch], b
    assert torch.equal(g.get_state(), runs[0][3])
    random.seed(3)
    for _ in sizes:
        random.random()
    assert random.getstate() == runs[0][4]                                  # one coin per item, nothing else
