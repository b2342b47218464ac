"""unmore_amd.roi_pool without a GPU: the restatement of tests/roi_pool_common.py pinned against independent statements of the same rule
(mask_loss_common's per-sample ROIAlign, F.grid_sample, plain average pooling, Detectron2's level rule worked by hand), and the
module's boundary: the import, the bound entry points, the header, the argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mask_loss_common import roi_align_average
from roi_pool_common import (assign_levels, axis_matrix, axis_samples, pooler_adjoint_np, pooler_np, pooler_rois, roi_align_adjoint_np,
                             roi_align_f32_np, roi_align_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _roi(box, image=0):
    return np.asarray([[image, *box]], dtype=np.float32)


@pytest.mark.parametrize("box", [(3.2, 4.7, 30.9, 21.3),            # inside the frame
                                 (11.0, 2.0, 25.0, 16.0),           # integer corners
                                 (-4.6, -2.3, 17.8, 9.9),           # across the top left corner
                                 (28.4, 15.5, 47.3, 29.8),          # across the bottom right corner
                                 (-9.5, -7.5, 49.1, 33.6),          # around the whole frame
                                 (20.3, 10.1, 20.9, 10.6),          # under one pixel
                                 (45.2, 3.3, 60.7, 20.1),           # wholly outside
                                 (9.0, 9.0, 9.0, 20.0)])            # zero width
@pytest.mark.parametrize("P", [7, 14])
def test_separable_form_equals_the_per_sample_rule_on_masks(box, P):
    rng = np.random.RandomState(3)
    mask = rng.uniform(size=(26, 40)) < 0.5
    want = roi_align_average(mask, np.asarray(box, dtype=np.float32), P, dtype=np.float64)
    got = roi_align_np(mask[None, None].astype(np.float32), _roi(box), P)[0, 0]
    assert np.abs(got - want).max() <= 1e-12
    if box[0] > 40:
        assert not got.any()                                            # every sample is further than one pixel outside


@pytest.mark.parametrize("P", [7, 14])
def test_separable_form_equals_grid_sample_and_a_2x2_mean(P):
    rng = np.random.RandomState(4)
    H, W, C, scale = 21, 33, 3, 0.5
    feat = rng.standard_normal((1, C, H, W))
    for box in [(6.3, 4.9, 50.2, 33.7), (10.0, 8.0, 38.0, 36.0), (20.4, 11.1, 23.0, 13.9)]:
        sy, sx = axis_samples(box[1], box[3], P, H, scale, 2), axis_samples(box[0], box[2], P, W, scale, 2)
        ys, xs = sy[0].reshape(-1), sx[0].reshape(-1)                   # [2P] coordinates, bin-major
        assert ys.min() >= 0 and ys.max() <= H - 1 and xs.min() >= 0 and xs.max() <= W - 1
        grid = torch.stack(torch.meshgrid(torch.from_numpy(2 * ys / (H - 1) - 1), torch.from_numpy(2 * xs / (W - 1) - 1), indexing="ij"), -1)
        sampled = F.grid_sample(torch.from_numpy(feat), grid.flip(-1)[None], mode="bilinear", align_corners=True)
        want = F.avg_pool2d(sampled, 2)[0].numpy()
        got = roi_align_np(feat, _roi(box), P, scale, 2)[0]             # float64 features are taken as they are
        assert got.shape == want.shape == (C, P, P)
        assert np.abs(got - want).max() <= 1e-12


def test_an_integer_box_is_plain_average_pooling():
    """[x0, y0, x0 + P k, y0 + P k] at scale 1: bin = grid = k and the sample (p, i) sits at x0 - .5 + p k + (i + .5) = x0 + p k + i, the
    centre of a pixel, so every tap weight is 1 or 0 and the bin is the mean of its k x k pixels"""
    rng = np.random.RandomState(5)
    feat = rng.standard_normal((1, 2, 30, 40))
    P, k, x0, y0 = 7, 3, 5, 4
    got = roi_align_np(feat, _roi((x0, y0, x0 + P * k, y0 + P * k)), P)[0]
    want = feat[0, :, y0:y0 + P * k, x0:x0 + P * k].reshape(2, P, k, P, k).mean(axis=(2, 4))
    assert np.abs(got - want).max() <= 1e-12
    A, grid = axis_matrix(x0, x0 + P * k, P, 40)
    assert grid == k and set(np.unique(A)) == {0.0, 1.0} and (A.sum(1) == k).all()
    got32 = roi_align_f32_np(feat, _roi((x0, y0, x0 + P * k, y0 + P * k)), P)[0]
    assert np.abs(got32 - want).max() <= 1e-6 * np.abs(feat).max()


def _square(side, x=3.0, y=5.0):
    return [x, y, x + side, y + side]


def test_level_rule_on_and_beside_the_boundaries():
    """canonical size 224 at level 4, levels 2..5: a side s lies on level floor(4 + log2(s / 224)), so 56 / 112 / 224 / 448 open the
    levels 2 / 3 / 4 / 5; below 56 clamps to 2 and 896 (level 6) clamps to 5.  Indices are levels minus 2."""
    sides = [28, 56, 112, 224, 448, 896]
    want = [0, 0, 1, 2, 3, 3]
    assert assign_levels([_square(s) for s in sides], 2, 5).tolist() == want
    below = assign_levels([_square(s - 0.5) for s in sides], 2, 5).tolist()
    above = assign_levels([_square(s + 0.5) for s in sides], 2, 5).tolist()
    assert below == [0, 0, 0, 1, 2, 3] and above == want
    assert assign_levels([[0, 0, 448, 112]], 2, 5).tolist() == [2]      # sqrt(448 * 112) = 224
    # a zero area, a negative area (NaN in the original), a NaN and a coordinate beyond 2^20: level 0
    odd = [[5, 5, 5, 90], [50, 5, 10, 90], [np.nan, 0, 300, 300], [0, 0, 3e6, 300]]
    assert assign_levels(odd, 2, 5).tolist() == [0, 0, 0, 0]
    assert assign_levels([_square(s) for s in (112, 224, 448)], 3, 4).tolist() == [0, 1, 1]
    assert assign_levels([_square(100)], 2, 5, canonical_box_size=100, canonical_level=3).tolist() == [1]


def test_adjoint_identity_of_the_restatement():
    rng = np.random.RandomState(6)
    P, shape = 7, (2, 3, 16, 24)
    feat, rois = rng.standard_normal(shape), np.asarray([[0, 2.2, 3.1, 40.3, 28.8], [1, -5.0, -3.0, 20.0, 40.0], [1, 30.2, 8.4, 60.5, 20.6],
                                                         [0, 9.0, 9.0, 9.0, 20.0], [0, np.nan, 0, 5, 5]], dtype=np.float32)
    for ratio in (0, 2):
        G = rng.standard_normal((len(rois), shape[1], P, P))
        lhs = (roi_align_np(feat, rois, P, 0.5, ratio) * G).sum()
        rhs = (feat * roi_align_adjoint_np(G, rois, shape, P, 0.5, ratio)).sum()
        assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0)
    boxes = [rois[:2, 1:] * 4, rois[2:4, 1:] * 4]
    maps = [rng.standard_normal((2, 3, 32 >> k, 48 >> k)) for k in range(3)]
    G = rng.standard_normal((4, 3, P, P))
    lhs = (pooler_np(maps, boxes, P, (0.25, 0.125, 0.0625)) * G).sum()
    rhs = sum((m * g).sum() for m, g in zip(maps, pooler_adjoint_np(G, [m.shape for m in maps], boxes, P, (0.25, 0.125, 0.0625))))
    assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0)
    assert pooler_rois(boxes)[:, 0].tolist() == [0, 0, 1, 1]


# ---- the module's boundary
ENTRY_POINTS = ("umr_roi_pool_prepare", "umr_roi_pool_forward", "umr_roi_pool_backward")


def test_module_imports_and_entry_points_are_bound():
    from unmore_amd import _lib as L
    from unmore_amd import roi_pool as R
    assert callable(R.roi_align) and callable(R.assign_boxes_to_levels) and issubclass(R.ROIPooler, torch.nn.Module)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    for name in ENTRY_POINTS:
        assert name in L.ARGTYPES and name not in L.RESTYPES
    assert L.ARGTYPES["umr_roi_pool_prepare"] == [vp, i32, i64, vp, i64, i32, i32, i32, f32, i32, vp, vp]
    assert L.ARGTYPES["umr_roi_pool_forward"] == [vp, i32, i64, i32, i32, vp, i32, vp, i64, i32, i32, vp, vp]
    assert L.ARGTYPES["umr_roi_pool_backward"] == [vp, i32, i64, i32, i32, vp, i32, vp, vp, i64, i32, i32, vp, vp]


def test_header_names_the_source_and_still_declares_ten_structs():
    text = open(os.path.join(ROOT, "include", "umr.h")).read()
    assert "csrc/roi_pool.hip" in text
    assert len(re.findall(r"typedef\s+struct\s+(umr_\w+)", text)) == 10
    assert os.path.exists(os.path.join(ROOT, "unmore_amd", "csrc", "roi_pool.hip"))


def _maps(dtype=torch.float32, n=2, c=3):
    return [torch.zeros((n, c, 32 >> k, 48 >> k), dtype=dtype) for k in range(4)]


def test_argument_errors_come_before_any_launch():
    from unmore_amd.roi_pool import ROIPooler, assign_boxes_to_levels, roi_align
    with pytest.raises(ValueError, match="ROIPool'"):
        ROIPooler(7, (0.25,), pooler_type="ROIPool")
    with pytest.raises(ValueError, match="ROIAlign'"):
        ROIPooler(7, (0.25,), pooler_type="ROIAlign")
    with pytest.raises(ValueError, match="consecutive powers of two"):
        ROIPooler(7, (0.25, 0.0625))
    with pytest.raises(ValueError, match="powers of two"):
        ROIPooler(7, (0.3, 0.15))
    with pytest.raises(ValueError, match="output_size"):
        ROIPooler((7, 14), (0.25,))
    with pytest.raises(ValueError, match="sampling_ratio"):
        ROIPooler(7, (0.25,), sampling_ratio=-1)
    pooler = ROIPooler(7, (0.25, 0.125, 0.0625, 0.03125), 0, "ROIAlignV2")
    assert (pooler.min_level, pooler.max_level) == (2, 5)
    boxes = [torch.zeros((3, 4)), torch.zeros((0, 4))]
    with pytest.raises(ValueError, match="3 level maps for 4 scales"):
        pooler(_maps()[:3], boxes)
    with pytest.raises(ValueError, match="1 box lists for 2 images"):
        pooler(_maps(), boxes[:1])
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        pooler(_maps(torch.float64), boxes)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        pooler(_maps(torch.float16), boxes)
    with pytest.raises(ValueError, match="same N, C and type"):
        pooler(_maps()[:3] + _maps(c=4)[3:], boxes)
    with pytest.raises(ValueError, match=r"box_lists\[0\] must be float32 \[R, 4\]"):
        pooler(_maps(), [torch.zeros((3, 5)), boxes[1]])
    with pytest.raises(ValueError, match=r"box_lists\[1\] must be float32"):
        pooler(_maps(), [boxes[0], torch.zeros((0, 4), dtype=torch.float64)])
    with pytest.raises(ValueError, match="aligned=True"):
        roi_align(_maps()[0], torch.zeros((1, 5)), 7, 0.25, aligned=False)
    with pytest.raises(ValueError, match=r"rois must be float32 \[R, 5\]"):
        roi_align(_maps()[0], torch.zeros((1, 4)), 7, 0.25)
    with pytest.raises(ValueError, match="spatial_scale"):
        roi_align(_maps()[0], torch.zeros((1, 5)), 7, 0.0)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        roi_align(_maps(torch.int32)[0], torch.zeros((1, 5)), 7, 0.25)
    with pytest.raises(ValueError, match="min_level"):
        assign_boxes_to_levels(torch.zeros((1, 4)), 3, 2)
    # well-formed arguments on the CPU: no fallback
    with pytest.raises(RuntimeError, match="MI355X only"):
        pooler(_maps(), boxes)
    with pytest.raises(RuntimeError, match="MI355X only"):
        roi_align(_maps()[0], torch.zeros((1, 5)), 7, 0.25)
    with pytest.raises(RuntimeError, match="MI355X only"):
        assign_boxes_to_levels(torch.zeros((1, 4)), 2, 5)
