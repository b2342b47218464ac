"""unmore_amd.roi_pool on the MI355X against the restatement of tests/roi_pool_common.py: a 128 x 192 frame under four levels (maps of
32 x 48 ... 4 x 6), two images, about 70 boxes that reach every branch (edge_case_boxes), P = 7 and 14, sampling ratio 0 and 2,
float32 and bfloat16, C = 3, 8 and 40 (the kernels work on chunks of 32 channels).

Allowances.  |device - float64 restatement| per element may be the larger of
  (a) the bound derived from the kernels' own order of operations: k 2^-24 (A |F| A^T / count) plus the weight-rounding term, with
      k = grid_h + grid_w + n_y + n_x + 8 forward (n: the most taps of a bin) and k = grid_h + grid_w + 8 + S backward (S: the adds a
      pixel can receive from the image's boxes); the derivations stand in roi_pool_common.forward_allowance / backward_allowance;
  (b) 4 x the largest error, on the same inputs, of the float32 restatement in torchvision's order (forward: sample by sample; backward:
      float32 weights and sums) against float64 -- another valid order may sit on the other side of the rounding.
bfloat16: the float64 restatement reads the bf16-rounded inputs, and the output's own rounding, 2^-8 relative, is added.
Input condition, asserted below on the float64 samples: no sample coordinate within 1e-3 of -1 or of the size (the rule's only
discontinuities), and float32 and float64 agree on every adaptive grid."""
import functools
import itertools

import numpy as np
import pytest
import torch

from roi_pool_common import (FRAME, STRIDES, assign_levels, backward_allowance, edge_case_boxes, forward_allowance, level_maps, pooler_rois,
                             roi_align_adjoint_f32_np, roi_align_adjoint_np, roi_align_f32_np, roi_align_np, sample_margin, tap_support)

pytestmark = pytest.mark.gpu

SCALES = tuple(1.0 / s for s in STRIDES)
N = 2
# (P, sampling ratio, dtype, C): every P x ratio x dtype, C cycling so that each C meets both types and both sides
CASES = [(P, ratio, dt, C) for (P, ratio, dt), C in zip(itertools.product((7, 14), (0, 2), ("float32", "bfloat16")), (3, 40, 8, 3, 40, 8, 3, 40))]
CASES += [(7, 0, "float32", 8), (14, 0, "bfloat16", 40)]
IDS = [f"P{p}-s{r}-{d}-C{c}" for p, r, d, c in CASES]


def _dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _rounded(a, dtype):
    """what the device reads: the array itself, or its bfloat16 rounding, as float32"""
    return a if dtype == "float32" else torch.from_numpy(a).to(torch.bfloat16).float().numpy()


def _t(a, dtype="float32"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev()).to(getattr(torch, dtype))


def _direct_rois():
    """roi_align on the finest map alone: the frame and a box around it (adaptive grids of 5 x 7 up to 10 x 12 at P = 7), boxes past every
    edge, the degenerate ones, a box of image 1, and two image indices the device refuses"""
    b = edge_case_boxes()
    rows = [[0, 0.0, 0.0, FRAME[1], FRAME[0]], [0, -64.3, -63.6, 256.7, 191.2], [1, 10.3, 20.6, 150.2, 100.9], [2, 10.3, 20.6, 50.2, 60.9],
            [0.5, 10.3, 20.6, 50.2, 60.9]]
    for name in ("beyond", "outside", "zero_width", "tiny", "nan"):
        rows += [[0, *box] for box in b[name]]
    return np.asarray(rows, dtype=np.float32)


def _check_inputs(rois, levels, P, ratio):
    for l, s in enumerate(STRIDES):
        margin, same = sample_margin(rois[levels == l], P, FRAME[0] // s, FRAME[1] // s, SCALES[l], ratio)
        assert margin >= 1e-3 and same, (l, margin, same)


def _limit(dev, ref, allow_a, err_b, dtype):
    allow = np.maximum(allow_a, 4 * err_b)
    if dtype == "bfloat16":
        allow = allow + 2.0 ** -8 * np.abs(ref)
    err = np.abs(dev - ref)
    print(f"max error {err.max():.3e}  allowance there {allow.reshape(-1)[err.argmax()]:.3e}  (a) max {allow_a.max():.3e}  (b) {4 * err_b:.3e}  "
          f"worst ratio {np.max(err / np.maximum(allow, 1e-300)):.3f}")
    return err, allow


@functools.lru_cache(maxsize=None)
def _run(P, ratio, dtype, C):
    """one case through the device and the restatement, shared by the tests below"""
    from unmore_amd.roi_pool import ROIPooler, roi_align
    rng = np.random.RandomState(100 + C)
    maps = [_rounded(m, dtype) for m in level_maps(rng, N, C)]
    boxes = [edge_case_boxes()["all"], np.zeros((0, 4), dtype=np.float32)]
    rois = pooler_rois(boxes)
    levels = assign_levels(rois[:, 1:], 2, 5)
    _check_inputs(rois, levels, P, ratio)
    R = len(rois)
    G = _rounded(rng.standard_normal((R, C, P, P)).astype(np.float32), dtype)
    x = [_t(m, dtype).requires_grad_(True) for m in maps]
    pooler = ROIPooler(P, SCALES, ratio, "ROIAlignV2")
    out = pooler(x, [_t(b) for b in boxes])
    out.backward(_t(G, dtype))
    grads = [t.grad.clone() for t in x]
    # roi_align on the finest map
    drois = _direct_rois()
    _check_inputs(drois, np.zeros(len(drois), dtype=np.int64), P, ratio)
    dG = _rounded(rng.standard_normal((len(drois), C, P, P)).astype(np.float32), dtype)
    x0 = _t(maps[0], dtype).requires_grad_(True)
    dout = roi_align(x0, _t(drois), P, SCALES[0], ratio)
    dout.backward(_t(dG, dtype))
    torch.cuda.synchronize()
    return {"maps": maps, "boxes": boxes, "rois": rois, "levels": levels, "G": G, "x": x, "pooler": pooler, "out": out,
            "grads": grads, "drois": drois, "dG": dG, "dout": dout, "dgrad": x0.grad.clone()}


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def test_levels_equal_the_float32_host_rule():
    from unmore_amd.roi_pool import assign_boxes_to_levels
    b = edge_case_boxes()
    got = assign_boxes_to_levels(_t(b["all"]), 2, 5).cpu().numpy()
    want = assign_levels(b["all"], 2, 5)
    assert got.dtype == np.int64 and (got == want).all()
    assert set(want.tolist()) == {0, 1, 2, 3}                           # every level is reached
    assert assign_levels(b["straddle"], 2, 5).tolist() == [0, 1, 1, 1, 2, 2, 2, 3, 3]
    sides = [[3, 5, 3 + s, 5 + s] for s in (28, 56, 112, 224, 448, 896, 55.5, 111.5, 223.5, 447.5, 56.5, 112.5, 224.5, 448.5)]
    got = assign_boxes_to_levels([_t(np.asarray(sides[:5], dtype=np.float32)), _t(np.asarray(sides[5:], dtype=np.float32))], 2, 5)
    assert got.cpu().tolist() == assign_levels(sides, 2, 5).tolist() == [0, 0, 1, 2, 3, 3, 0, 0, 1, 2, 0, 1, 2, 3]
    assert assign_boxes_to_levels(_t(np.asarray(sides, dtype=np.float32)), 3, 4).cpu().tolist() == assign_levels(sides, 3, 4).tolist()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_against_float64(case):
    P, ratio, dtype, C = case
    run = _run(*case)
    # the pooler: every box on the map of its level
    ref = np.zeros((len(run["rois"]), C, P, P))
    allow_a, err_b = np.zeros_like(ref), 0.0
    for l in range(4):
        pick = run["levels"] == l
        args = (run["maps"][l], run["rois"][pick], P, SCALES[l], ratio)
        ref[pick] = roi_align_np(*args)
        allow_a[pick] = forward_allowance(*args)
        err_b = max(err_b, np.abs(roi_align_f32_np(*args) - ref[pick]).max())
    out = _np64(run["out"])
    assert run["out"].dtype == getattr(torch, dtype) and out.shape == ref.shape
    err, allow = _limit(out, ref, allow_a, err_b, dtype)
    assert (err <= allow).all()
    # refused and empty boxes: zero rows, exactly
    b, at, row = edge_case_boxes(), {}, 0
    for name in ("straddle", "beyond", "outside", "zero_width", "tiny", "huge", "nan"):       # the order of edge_case_boxes()["all"]
        at[name], row = row, row + len(b[name])
    for name in ("outside", "zero_width", "nan"):
        assert not out[at[name]].any() and not ref[at[name]].any(), name
    assert np.abs(ref[at["tiny"]]).max() > 0 and np.abs(ref[at["huge"]]).max() > 0
    # roi_align on the finest map: any footprint, any grid
    args = (run["maps"][0], run["drois"], P, SCALES[0], ratio)
    dref = roi_align_np(*args)
    derr, dallow = _limit(_np64(run["dout"]), dref, forward_allowance(*args), np.abs(roi_align_f32_np(*args) - dref).max(), dtype)
    assert (derr <= dallow).all()
    assert not _np64(run["dout"])[3:5].any()                            # image index 2 of 2 images, image index 0.5
    assert np.abs(dref[2]).max() > 0                                    # the box of image 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_against_the_float64_adjoint(case):
    P, ratio, dtype, C = case
    run = _run(*case)
    for l in range(4):
        pick = run["levels"] == l
        shape = run["maps"][l].shape
        args = (run["G"][pick], run["rois"][pick], shape, P, SCALES[l], ratio)
        ref = roi_align_adjoint_np(*args)
        got = _np64(run["grads"][l])
        assert run["grads"][l].dtype == getattr(torch, dtype)
        err, allow = _limit(got, ref, backward_allowance(*args), np.abs(roi_align_adjoint_f32_np(*args) - ref).max(), dtype)
        assert (err <= allow).all(), l
        support = tap_support(run["rois"][pick], shape, P, SCALES[l], ratio)
        assert not got.transpose(0, 2, 3, 1)[~support].any(), l          # exactly zero wherever no tap lands
        assert not got[1].any()                                          # image 1 has no boxes
    shape = run["maps"][0].shape
    args = (run["dG"], run["drois"], shape, P, SCALES[0], ratio)
    ref = roi_align_adjoint_np(*args)
    err, allow = _limit(_np64(run["dgrad"]), ref, backward_allowance(*args), np.abs(roi_align_adjoint_f32_np(*args) - ref).max(), dtype)
    assert (err <= allow).all()
    assert np.abs(ref[1]).max() > 0


@pytest.mark.parametrize("case", [CASES[0], CASES[5], CASES[9]], ids=[IDS[0], IDS[5], IDS[9]])
def test_pooler_equals_per_level_roi_align_bit_for_bit(case):
    from unmore_amd.roi_pool import assign_boxes_to_levels, roi_align
    P, ratio, dtype, C = case
    run = _run(*case)
    rois = _t(run["rois"])
    levels = assign_boxes_to_levels([_t(b) for b in run["boxes"]], 2, 5).cpu()
    want = torch.zeros_like(run["out"])
    for l in range(4):
        pick = torch.nonzero(levels == l)[:, 0].to(_dev())
        want[pick] = roi_align(run["x"][l].detach(), rois[pick], P, SCALES[l], ratio)
    assert torch.equal(run["out"], want)


def test_boxes_in_both_images_and_empty_levels():
    """the second case: boxes in both images (a wrong image index would show), none on the two coarsest levels, an empty image between"""
    from unmore_amd.roi_pool import ROIPooler
    P, C = 7, 8
    rng = np.random.RandomState(7)
    maps = level_maps(rng, 3, C)
    b = edge_case_boxes()
    boxes = [np.concatenate([b["beyond"], b["tiny"], b["straddle"][:3]]), np.zeros((0, 4), dtype=np.float32),
             np.concatenate([b["copies"][:3], b["random"], b["straddle"][:2], b["nan"]])]
    rois = pooler_rois(boxes)
    levels = assign_levels(rois[:, 1:], 2, 5)
    assert set(levels.tolist()) == {0, 1}
    _check_inputs(rois, levels, P, 0)
    G = rng.standard_normal((len(rois), C, P, P)).astype(np.float32)
    x = [_t(m).requires_grad_(True) for m in maps]
    out = ROIPooler(P, SCALES)(x, [_t(v) for v in boxes])
    out.backward(_t(G))
    for l in range(4):
        pick = levels == l
        if pick.any():
            args = (maps[l], rois[pick], P, SCALES[l], 0)
            ref = roi_align_np(*args)
            err, allow = _limit(_np64(out)[pick], ref, forward_allowance(*args), np.abs(roi_align_f32_np(*args) - ref).max(), "float32")
            assert (err <= allow).all()
        args = (G[pick], rois[pick], maps[l].shape, P, SCALES[l], 0)
        gref = roi_align_adjoint_np(*args)
        got = _np64(x[l].grad)
        gerr, gallow = _limit(got, gref, backward_allowance(*args), np.abs(roi_align_adjoint_f32_np(*args) - gref).max(), "float32")
        assert (gerr <= gallow).all()
        assert not got[1].any()
        if l >= 2:
            assert not got.any()                                         # no box was assigned to this level: written, and zero
    assert np.abs(_np64(x[0].grad)[2]).max() > 0 and np.abs(_np64(x[0].grad)[0]).max() > 0


def test_fifty_copies_give_fifty_times_one_copy():
    from unmore_amd.roi_pool import ROIPooler
    P, C = 7, 8
    rng = np.random.RandomState(8)
    maps = level_maps(rng, 1, C)
    box = edge_case_boxes()["copies"][:1]
    g1 = rng.standard_normal((1, C, P, P)).astype(np.float32)
    grads = {}
    for n in (1, 50):
        x = [_t(m).requires_grad_(True) for m in maps]
        ROIPooler(P, SCALES)(x, [_t(np.repeat(box, n, 0))]).backward(_t(np.repeat(g1, n, 0)))
        grads[n] = [_np64(t.grad) for t in x]
    l = int(assign_levels(box, 2, 5)[0])
    rois = pooler_rois([np.repeat(box, 50, 0)])
    allow50 = backward_allowance(np.repeat(g1, 50, 0), rois, maps[l].shape, P, SCALES[l], 0)
    allow1 = backward_allowance(g1, rois[:1], maps[l].shape, P, SCALES[l], 0)
    err = np.abs(grads[50][l] - 50 * grads[1][l])
    print(f"max |g50 - 50 g1| {err.max():.3e}  allowance there {(allow50 + 50 * allow1).reshape(-1)[err.argmax()]:.3e}")
    assert np.abs(grads[1][l]).max() > 0 and (err <= allow50 + 50 * allow1).all()
    for k in range(4):
        if k != l:
            assert not grads[50][k].any()


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_device_adjoint_identity(case):
    """<A F, G> = <F, A^T G> between the two device kernels, in float64, within the summed allowances of both sides"""
    P, ratio, dtype, C = case
    run = _run(*case)
    lhs = (_np64(run["out"]) * run["G"]).sum()
    rhs = sum((_np64(g) * m).sum() for g, m in zip(run["grads"], run["maps"]))
    slack = 0.0
    for l in range(4):
        pick = run["levels"] == l
        fa = forward_allowance(run["maps"][l], run["rois"][pick], P, SCALES[l], ratio)
        fb = np.abs(roi_align_f32_np(run["maps"][l], run["rois"][pick], P, SCALES[l], ratio)
                    - roi_align_np(run["maps"][l], run["rois"][pick], P, SCALES[l], ratio)).max()
        slack += (np.maximum(fa, 4 * fb) * np.abs(run["G"][pick])).sum()
        args = (run["G"][pick], run["rois"][pick], run["maps"][l].shape, P, SCALES[l], ratio)
        bb = np.abs(roi_align_adjoint_f32_np(*args) - roi_align_adjoint_np(*args)).max()
        slack += (np.maximum(backward_allowance(*args), 4 * bb) * np.abs(run["maps"][l])).sum()
    print(f"<AF,G> {lhs:.9e}  <F,A'G> {rhs:.9e}  difference {abs(lhs - rhs):.3e}  allowance {slack:.3e}")
    assert abs(lhs - rhs) <= slack


@pytest.mark.parametrize("case", [CASES[0], CASES[7]], ids=[IDS[0], IDS[7]])
def test_same_input_same_bytes(case):
    P, ratio, dtype, C = case
    run = _run(*case)
    for _ in range(2):
        x = [t.detach().clone().requires_grad_(True) for t in run["x"]]
        out = run["pooler"](x, [_t(b) for b in run["boxes"]])
        out.backward(_t(run["G"], dtype))
        assert torch.equal(out, run["out"])
        for g, t in zip(run["grads"], x):
            assert torch.equal(g, t.grad)


def test_a_box_over_a_whole_larger_map():
    """a footprint of 50 x 70 pixels and an adaptive grid of 8 x 10 (nothing caps either), beside a small box of the other image; forward
    and backward, the backward over several tiles per box"""
    from unmore_amd.roi_pool import roi_align
    P, C = 7, 5
    rng = np.random.RandomState(9)
    feat = rng.standard_normal((2, C, 50, 70)).astype(np.float32)
    rois = np.asarray([[1, -0.7, -0.4, 70.6, 50.3], [0, 10.3, 8.2, 30.9, 25.6], [1, 3.1, 2.2, 66.4, 47.7]], dtype=np.float32)
    margin, same = sample_margin(rois, P, 50, 70, 1.0, 0)
    assert margin >= 1e-3 and same
    G = rng.standard_normal((3, C, P, P)).astype(np.float32)
    x = _t(feat).requires_grad_(True)
    out = roi_align(x, _t(rois), P, 1.0, 0)
    out.backward(_t(G))
    args = (feat, rois, P, 1.0, 0)
    ref = roi_align_np(*args)
    err, allow = _limit(_np64(out), ref, forward_allowance(*args), np.abs(roi_align_f32_np(*args) - ref).max(), "float32")
    assert (err <= allow).all()
    args = (G, rois, feat.shape, P, 1.0, 0)
    gref = roi_align_adjoint_np(*args)
    gerr, gallow = _limit(_np64(x.grad), gref, backward_allowance(*args), np.abs(roi_align_adjoint_f32_np(*args) - gref).max(), "float32")
    assert (gerr <= gallow).all()


def test_no_boxes_no_launch():
    from unmore_amd import _lib as L
    from unmore_amd.roi_pool import ROIPooler, roi_align
    maps = [_t(m) for m in level_maps(np.random.RandomState(0), 2, 3)]
    before = L._count[0]
    out = ROIPooler(7, SCALES)(maps, [_t(np.zeros((0, 4), dtype=np.float32))] * 2)
    assert tuple(out.shape) == (0, 3, 7, 7) and out.dtype == torch.float32
    out = roi_align(maps[0].to(torch.bfloat16), _t(np.zeros((0, 5), dtype=np.float32)), 14, 0.25)
    assert tuple(out.shape) == (0, 3, 14, 14) and out.dtype == torch.bfloat16
    assert L._count[0] == before
