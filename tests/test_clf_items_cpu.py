"""The existence classifier's training item and evaluation without a GPU: the zero-border shortcut the kernel relies on
equals the reference's padded transform, the new entry points are declared, bound, exported and reject bad arguments before
any HIP call, and the host entry points refuse CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import labels_oracle as LO

import clf_items_common as C

NEW = ("umr_bg_square", "umr_bg_square_workspace", "umr_crop_resize_ragged")


def _edge_masks():
    """(name, full mask u8): the cases the background branch has to get right"""
    out = []
    m = np.zeros((17, 23), np.uint8)
    out.append(("empty mask: everything is background", m))
    out.append(("no background at all", np.full((9, 14), 255, np.uint8)))
    m = np.full((12, 10), 1, np.uint8)
    m[:, 0] = 0
    out.append(("background one pixel thin along the left edge", m))
    m = np.full((10, 12), 7, np.uint8)
    m[0, :] = 0
    out.append(("background one pixel thin along the top edge", m))
    m = np.full((15, 31), 200, np.uint8)
    m[3:10, 2:9] = 0
    m[3:10, 20:27] = 0
    out.append(("two equal background squares: first maximum in raster order", m))
    out.append(("one column", np.zeros((33, 1), np.uint8)))
    out.append(("one pixel of background", np.array([[0]], np.uint8)))
    return out


def _random_masks(n, rng, max_side=40):
    for _ in range(n):
        h, w = int(rng.integers(1, max_side + 1)), int(rng.integers(1, max_side + 1))
        yield (rng.random((h, w)) < rng.uniform(0.05, 0.95)).astype(np.uint8) * 255


def test_padding_ten_equals_padding_one_equals_the_zero_border():
    """datasets.py:305-307 pads the background mask with ten rings of zeros before cv2.distanceTransform.  One ring gives the
    same field, and so does the transform with its border initialised to 0 on the unpadded mask (what umr_bg_square runs):
    field, argmax and box agree bit for bit, with the literal raster passes and with the scan form."""
    rng = np.random.default_rng(20)
    masks = [m for _, m in _edge_masks()] + list(_random_masks(30, rng))
    for m in masks:
        bg = (1 - (m > 0)).astype(np.uint8)
        f10 = LO.distance_transform_3x3_literal(np.pad(bg, 10))[10:-10, 10:-10]
        f1 = LO.distance_transform_3x3_literal(np.pad(bg, 1))[1:-1, 1:-1]
        f10s = LO.distance_transform_3x3(np.pad(bg, 10))[10:-10, 10:-10]
        fz = C.zero_border_field(bg)
        assert f10.dtype == f1.dtype == fz.dtype == np.float32
        assert np.array_equal(f10, f1) and np.array_equal(f10, f10s) and np.array_equal(f10, fz), m.shape
        b10 = C.bg_square(m, 10, LO.distance_transform_3x3_literal)
        assert b10 == C.bg_square(m, 1, LO.distance_transform_3x3_literal) == C.bg_square(m, 10)
        h, w = m.shape
        x1, y1, x2, y2 = b10
        assert 0 <= x1 <= w and 0 <= x2 <= w and 0 <= y1 <= h and 0 <= y2 <= h, (b10, m.shape)      # every box lies inside its image
        assert C.bg_square_zero_border(m) == (x1, y1, x2, y2, int(x2 > x1 and y2 > y1))


def test_edge_cases_of_the_background_branch():
    cases = dict(_edge_masks())
    assert C.bg_square_zero_border(cases["no background at all"]) == (0, 0, 0, 0, 0)
    # a maximum of 0.955 in column 0: x1 = int(0 - 0.955) = 0 = x2 = int(0.955) -> zero-width slice
    x1, y1, x2, y2, ok = C.bg_square_zero_border(cases["background one pixel thin along the left edge"])
    assert (x1, x2, ok) == (0, 0, 0)
    x1, y1, x2, y2, ok = C.bg_square_zero_border(cases["background one pixel thin along the top edge"])
    assert (y1, y2, ok) == (0, 0, 0)
    # 17 x 23, all background: the field peaks at row 8 (9 pixels from either edge), first at column 8
    assert C.bg_square_zero_border(cases["empty mask: everything is background"]) == (0, 0, 16, 16, 1)
    # two equal 7 x 7 squares: the left one (lower raster index) wins -- centre (x 5, y 6), r = 4 * 0.955 = 3.82
    assert C.bg_square_zero_border(cases["two equal background squares: first maximum in raster order"]) == (1, 2, 8, 9, 1)
    # an empty crop falls through to the foreground branch in the item restatement
    img = torch.rand(3, 12, 10, generator=torch.Generator().manual_seed(0))
    top1 = torch.full((12, 10), 255, dtype=torch.uint8)
    full = torch.from_numpy(cases["background one pixel thin along the left edge"])
    out, label, info = C.classifier_item(img, top1, full, True, (0, 0, 12, 10), 8)
    assert info["branch"] == 1 and label == 1.0 and out.shape == (3, 8, 8)
    out, label, info = C.classifier_item(img, top1, torch.zeros(12, 10, dtype=torch.uint8), True, None, 8)
    # 12 x 10, all background: r = 5 * 0.955 = 4.775 first at (y 4, x 4) -> int(-0.775) = 0, int(8.775) = 8
    assert info["branch"] == 0 and label == 0.0 and info["box"] == (0, 0, 8, 8)


def test_new_entry_points_are_declared_bound_and_exported():
    from unmore_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "umr.h")).read()
    declared = set(re.findall(r"\b(umr_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared
    assert set(NEW) <= set(_lib.exported_symbols())
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), f"{name} is not exported by the built library"
    assert ctypes.sizeof(_lib.RaggedSrc) == 24      # umr_ragged_src: two pointers, two int32


def _expect(status, code, what):
    from unmore_amd import _lib
    assert status == code, (what, status)
    msg = _lib.lib().umr_last_error_string().decode()
    assert msg, what
    return msg


def test_argument_errors_without_a_gpu():
    from unmore_amd import _lib
    lib = _lib.lib()
    INVALID, UNSUPPORTED = -1, -2
    buf = (ctypes.c_int32 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.umr_bg_square_workspace(0, 100) == 0 and lib.umr_bg_square_workspace(3, 0) == 0
    assert lib.umr_bg_square_workspace(3, 500 * 375) == 3 * 500 * 375 * 4
    big = 1 << 40
    assert "null" in _expect(lib.umr_bg_square(None, p, p, big, 2, 500, 500 * 375, None), INVALID, "null table")
    assert "null" in _expect(lib.umr_bg_square(p, None, p, big, 2, 500, 500 * 375, None), INVALID, "null output")
    assert "null" in _expect(lib.umr_bg_square(p, p, None, big, 2, 500, 500 * 375, None), INVALID, "null workspace")
    assert "geometry" in _expect(lib.umr_bg_square(p, p, p, big, 0, 500, 500 * 375, None), INVALID, "B = 0")
    assert "geometry" in _expect(lib.umr_bg_square(p, p, p, big, -3, 500, 500 * 375, None), INVALID, "B < 0")
    assert "geometry" in _expect(lib.umr_bg_square(p, p, p, big, 2, 500, 499, None), INVALID, "max_pixels < max_w")
    assert "workspace" in _expect(lib.umr_bg_square(p, p, p, 2 * 500 * 375 * 4 - 1, 2, 500, 500 * 375, None), INVALID, "workspace")
    assert "4096" in _expect(lib.umr_bg_square(p, p, p, big, 2, 4097, 4097 * 10, None), UNSUPPORTED, "row wider than the limit")
    assert "null" in _expect(lib.umr_crop_resize_ragged(None, p, p, p, p, 2, 3, 8, 8, None), INVALID, "null table")
    assert "null" in _expect(lib.umr_crop_resize_ragged(p, None, p, p, p, 2, 3, 8, 8, None), INVALID, "null boxes")
    assert "null" in _expect(lib.umr_crop_resize_ragged(p, p, None, p, p, 2, 3, 8, 8, None), INVALID, "null dst")
    assert "mask" in _expect(lib.umr_crop_resize_ragged(p, p, p, p, None, 2, 3, 8, 8, None), INVALID, "mask_out without mask_sum")
    assert "mask" in _expect(lib.umr_crop_resize_ragged(p, p, p, None, p, 2, 3, 8, 8, None), INVALID, "mask_sum without mask_out")
    assert "geometry" in _expect(lib.umr_crop_resize_ragged(p, p, p, p, p, 0, 3, 8, 8, None), INVALID, "B = 0")
    assert "geometry" in _expect(lib.umr_crop_resize_ragged(p, p, p, None, None, 2, 0, 8, 8, None), INVALID, "C = 0")
    assert "geometry" in _expect(lib.umr_crop_resize_ragged(p, p, p, None, None, 2, 3, 8, 0, None), INVALID, "Wo = 0")


def test_host_entry_points_refuse_cpu_tensors():
    from unmore_amd import ClassifierTrainStep, synthesize_classifier_items
    from unmore_amd.binary_classifier import Binary_Classifier
    img = torch.zeros(3, 8, 8)
    m = torch.zeros(8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        synthesize_classifier_items([img], [m], [m], 8, coins=[True])
    # evaluate: a step cannot be constructed around a CPU model, so the method runs on a bare instance holding one
    step = object.__new__(ClassifierTrainStep)
    step.net = Binary_Classifier(device="cpu", image_size=64, args=None)
    for mode in (True, False):
        step.net.train(mode)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            step.evaluate([(torch.zeros(2, 3, 64, 64), torch.zeros(2, 1))])
        assert step.net.training is mode        # restored after the raising batch
