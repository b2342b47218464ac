"""The NumPy restatement of the RPN proposal step (tests/rpn_common.py) pinned without a GPU -- hand-worked values, torch.topk,
box_loss_common's decode and a plain torch-CPU composition of the whole step -- so that the GPU tests rest on something; and every
host check of unmore_amd.rpn that needs no device."""
import numpy as np
import pytest
import torch

import rpn_common as C
from box_loss_common import apply_deltas_np
from unmore_amd import _lib as L
from unmore_amd import rpn

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- anchors
def test_cell_anchors_hand_worked():
    (got,) = rpn.cell_anchors([[32]], [0.5, 1.0, 2.0])
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4)
    a, b = F32(22.627417), F32(11.313708)
    want = np.array([[-a, -b, a, b], [-16, -16, 16, 16], [-b, -a, b, a]], dtype=F32)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(C.cell_anchors_np((32,), (0.5, 1.0, 2.0)), want)
    # one ratio list is broadcast over the levels; sizes within a level come first
    per = rpn.cell_anchors([[32], [64, 128]], [0.5, 1.0, 2.0])
    assert [tuple(p.shape) for p in per] == [(3, 4), (6, 4)]
    assert np.array_equal(per[1].numpy(), C.cell_anchors_np((64, 128), (0.5, 1.0, 2.0)))
    assert np.array_equal(per[1][3:].numpy(), (want * 4).astype(F32))
    assert np.array_equal(rpn.cell_anchors([[32], [64]], [[1.0], [2.0]])[1].numpy(), C.cell_anchors_np((64,), (2.0,)))


def test_grid_anchors_order_and_values():
    cells = rpn.cell_anchors([[32]], [0.5, 1.0, 2.0])
    (got,) = rpn.grid_anchors(cells, [8], [(2, 3)], offset=0.5)
    assert tuple(got.shape) == (18, 4) and got.dtype == torch.float32
    c = cells[0].numpy()
    f = 0
    for y in range(2):
        for x in range(3):
            for a in range(3):
                sx, sy = F32(x * 8 + 4), F32(y * 8 + 4)
                assert np.array_equal(got[f].numpy(), np.array([sx + c[a, 0], sy + c[a, 1], sx + c[a, 2], sy + c[a, 3]], dtype=F32)), f
                f += 1
    assert np.array_equal(got.numpy(), C.anchors_np(c, 8, 2, 3, 0.5))
    assert np.array_equal(rpn.grid_anchors(cells, [8], [(2, 3)])[0][0].numpy(), c[0])       # offset 0: the first anchor is the cell


# ---------------------------------------------------------------------------------------------------------------- top-k
def test_topk_equals_torch_on_tie_free_input():
    rng = np.random.RandomState(0)
    v = rng.permutation(5000).astype(F32) * F32(0.37) - F32(900)
    for k in (1, 64, 777, 5000, 6000):
        want = torch.topk(torch.from_numpy(v), min(k, len(v)), sorted=True)
        got = C.topk_np(v, k)
        assert np.array_equal(got, want.indices.numpy()), k
        assert np.array_equal(v[got], want.values.numpy())


def test_topk_ties_zeros_and_nan_hand_worked():
    inf, nan = np.inf, np.nan
    #              0    1     2    3    4     5    6    7    8
    v = np.array([1.0, 2.0, -0.0, 2.0, nan, 0.0, inf, 2.0, nan], dtype=F32)
    assert C.topk_np(v, 9).tolist() == [4, 8, 6, 1, 3, 7, 0, 2, 5]      # NaN above +inf; equal values by index; -0.0 == +0.0 by index
    assert C.topk_np(v, 4).tolist() == [4, 8, 6, 1]
    assert C.topk_np(v, 5).tolist() == [4, 8, 6, 1, 3]                  # the tied k-th value: the lower index
    assert C.topk_np(np.array([0.0, -0.0, -1.0, -inf], dtype=F32), 3).tolist() == [0, 1, 2]
    k = C.order_keys(np.array([-inf, -1.0, -0.0, 0.0, 1e-45, 1.0, inf, nan], dtype=F32)).astype(np.int64)
    assert (np.diff(k) >= 0).all() and k[2] == k[3] and (np.diff(k)[[0, 1, 3, 4, 5, 6]] > 0).all()
    # torch.topk agrees about the values
    want = torch.topk(torch.from_numpy(v), 5).values.numpy()
    assert np.array_equal(np.isnan(want), np.isnan(v[C.topk_np(v, 5)])) and np.array_equal(want[2:], v[C.topk_np(v, 5)][2:])


def test_flat_index_is_y_x_a():
    z = np.arange(2 * 3 * 4, dtype=F32).reshape(2, 3, 4)                # [A, H, W]
    flat = C.flat_scores(z)
    for a in range(2):
        for y in range(3):
            for x in range(4):
                assert flat[(y * 4 + x) * 2 + a] == z[a, y, x]
    d = np.arange(8 * 3 * 4, dtype=F32).reshape(8, 3, 4)                # [4A, H, W], channel a * 4 + c
    got = C.gather_deltas(d, [(1 * 4 + 2) * 2 + 1], 2)
    assert np.array_equal(got, np.array([[d[4 + c, 1, 2] for c in range(4)]], dtype=F32))


# ---------------------------------------------------------------------------------------------------------------- decode
def test_decode_equals_box_loss_restatement():
    rng = np.random.RandomState(1)
    anchors = C.anchors_np(C.cell_anchors_np((32,), (0.5, 1.0, 2.0)), 4, 20, 30)
    deltas = (rng.standard_normal((len(anchors), 4)) * 0.5).astype(F32)
    deltas[::7, 2], deltas[::11, 3], deltas[5, 0] = 6.0, 50.0, np.nan   # past the clamp; a NaN stays
    for w in ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)):
        for dt in (np.float32, np.float64):
            got, want = C.decode_np(deltas, anchors, w, dt), apply_deltas_np(deltas, anchors, w, dt)
            assert got.dtype == dt and np.array_equal(got, want, equal_nan=True)
    out = C.decode_np(deltas, anchors)
    assert np.isnan(out[5]).tolist() == [True, False, True, False] and np.isfinite(out[11::11]).all()


# ---------------------------------------------------------------------------------------------------------------- NMS and merge
def test_flags_clip_and_min_box_size():
    raw = np.array([[-5, -5, 10, 10], [50, 5, 70, 8], [1, 1, 4, 4], [2, 2, np.inf, 3], [1, 1, 1, 9], [0, 0, 3, 3]], dtype=F32)
    box, fl = C.flags_np(raw, np.array([1, 1, 1, 1, 1, np.nan], F32), 20, 40, 0.0)
    assert np.array_equal(box[0], [0, 0, 10, 10]) and np.array_equal(box[1], [40, 5, 40, 8])
    assert fl.tolist() == [0, 2, 0, 1, 2, 1]                            # clipped to zero width; non-finite box; zero width; NaN logit
    assert C.flags_np(raw, np.ones(6, F32), 20, 40, 3.0)[1].tolist() == [0, 2, 2, 1, 2, 2]       # strictly greater than min_box_size


def test_nms_and_merge_hand_worked():
    a, b, c = [0, 0, 10, 10], [0, 0, 10, 8], [20, 20, 30, 30]           # iou(a, b) = 0.8
    boxes = np.array([a, b, c, a], dtype=F32)
    assert C.iou_row(boxes[0], boxes[1:]).tolist() == [F32(0.8), 0, 1]
    assert C.nms_np(boxes, [0, 0, 0, 0], 0.65).tolist() == [0, 2]
    assert C.nms_np(boxes, [0, 0, 0, 0], 0.8).tolist() == [0, 1, 2]     # iou == thresh does not suppress
    assert C.nms_np(boxes, [2, 0, 0, 0], 0.65).tolist() == [1, 2]       # a dropped candidate suppresses nothing: b lives, a (rank 3) dies by b
    assert C.nms_np(np.zeros((2, 4), F32), [0, 0], 0.1).tolist() == [0, 1]                      # 0 / 0: not suppressed
    # two levels with identical boxes: neither suppresses the other; an equal logit orders by level, then rank
    lb = [boxes[[0, 2]], boxes[[0, 2]]]
    ls = [np.array([2.0, 1.0], F32), np.array([2.0, 1.5], F32)]
    out_b, out_s, cnt = C.finish_np(lb, ls, [[0, 0], [0, 0]], 0.65, 10)
    assert out_s.tolist() == [2.0, 2.0, 1.5, 1.0] and cnt.tolist() == [[2, 0, 0, 0, 2], [2, 0, 0, 0, 2]]
    assert np.array_equal(out_b, np.array([a, a, c, c], dtype=F32))
    lv, at = C.merge_np(ls, 10)
    assert lv.tolist() == [0, 1, 1, 0] and at.tolist() == [0, 0, 1, 1]
    assert C.merge_np([np.array([0.0], F32), np.array([-0.0], F32)], 5)[0].tolist() == [0, 1]   # -0.0 == +0.0: by level
    assert C.merge_np([np.array([-0.0], F32), np.array([0.0], F32)], 5)[0].tolist() == [0, 1]
    # truncation by post_nms_topk
    out_b, out_s, _ = C.finish_np(lb, ls, [[0, 0], [0, 0]], 0.65, 3)
    assert out_s.tolist() == [2.0, 2.0, 1.5] and len(out_b) == 3
    assert C.finish_np([np.zeros((0, 4), F32)], [np.zeros(0, F32)], [np.zeros(0, np.uint8)], 0.5, 3)[0].shape == (0, 4)


# ---------------------------------------------------------------------------------------------------------------- the whole step
def _torch_composition(logits, deltas, cells, strides, image_sizes, thresh, pre, post, min_box, offset):
    """find_top_rpn_proposals as plain torch-CPU ops, NMS as a greedy loop per level (torchvision is not needed)"""
    N = logits[0].shape[0]
    anchors = rpn.grid_anchors(cells, strides, [tuple(s.shape[2:]) for s in logits], offset)
    per_level = []
    for s, d, an in zip(logits, deltas, anchors):
        A, H, W = s.shape[1:]
        sc = s.permute(0, 2, 3, 1).flatten(1)
        dl = d.view(N, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, 4)
        k = min(pre, sc.shape[1])
        top, idx = sc.topk(k, dim=1)
        rows = []
        for n in range(N):
            a, t = an[idx[n]], dl[n, idx[n]]
            w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
            cx, cy = a[:, 0] + 0.5 * w, a[:, 1] + 0.5 * h
            dw, dh = torch.clamp(t[:, 2], max=C.SCALE_CLAMP), torch.clamp(t[:, 3], max=C.SCALE_CLAMP)
            pcx, pcy = t[:, 0] * w + cx, t[:, 1] * h + cy
            pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
            rows.append(torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], dim=1))
        per_level.append((top, rows))
    out = []
    for n, (h, w) in enumerate(image_sizes):
        kept_b, kept_s, kept_l = [], [], []
        for l, (top, rows) in enumerate(per_level):
            b, s = rows[n], top[n]
            ok = torch.isfinite(b).all(dim=1) & torch.isfinite(s)
            b, s = b[ok], s[ok]
            b = torch.stack([b[:, 0].clamp(0, w), b[:, 1].clamp(0, h), b[:, 2].clamp(0, w), b[:, 3].clamp(0, h)], dim=1)
            ok = ((b[:, 2] - b[:, 0]) > min_box) & ((b[:, 3] - b[:, 1]) > min_box)
            b, s = b[ok], s[ok]
            keep = []
            area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
            for i in range(len(b)):
                if keep:
                    kb = b[keep]
                    iw = (torch.minimum(kb[:, 2], b[i, 2]) - torch.maximum(kb[:, 0], b[i, 0])).clamp(min=0)
                    ih = (torch.minimum(kb[:, 3], b[i, 3]) - torch.maximum(kb[:, 1], b[i, 1])).clamp(min=0)
                    inter = iw * ih
                    if ((inter / ((area[keep] + area[i]) - inter)) > thresh).any():
                        continue
                keep.append(i)
            kept_b.append(b[keep]), kept_s.append(s[keep]), kept_l.append(torch.full((len(keep),), l))
        b, s = torch.cat(kept_b), torch.cat(kept_s)
        order = torch.sort(s, descending=True, stable=True).indices[:post]
        out.append((b[order].numpy(), s[order].numpy()))
    return out


def test_whole_restatement_equals_a_torch_composition():
    """tie-free logits (a permutation), exact decodes aside: the restatement's float32 steps are torch's float32 steps, so the kept
    sets and orders are equal; the boxes are compared to 2 ulp of the frame because torch.exp and np.exp need not round alike"""
    rng = np.random.RandomState(5)
    N, A, strides, maps = 2, 3, (4, 8, 16), ((12, 17), (6, 9), (3, 5))
    cells = rpn.cell_anchors([[16], [32], [64]], [0.5, 1.0, 2.0])
    total = sum(N * A * h * w for h, w in maps)
    perm = (rng.permutation(total).astype(F32) - F32(total / 2)) * F32(0.01)
    logits, deltas, at = [], [], 0
    for h, w in maps:
        n = N * A * h * w
        logits.append(perm[at:at + n].reshape(N, A, h, w))
        deltas.append((rng.standard_normal((N, 4 * A, h, w)) * 0.2).astype(F32))
        at += n
    sizes = [(48, 68), (24, 30)]
    want = _torch_composition([torch.from_numpy(x) for x in logits], [torch.from_numpy(x) for x in deltas], cells, strides, sizes, 0.65,
                              150, 120, 2.0, 0.5)
    got = C.proposals_np(logits, deltas, [c.numpy() for c in cells], strides, sizes, 0.65, 150, 120, 2.0, offset=0.5)
    assert len(got[0]["boxes"]) == 120 and 0 < len(got[1]["boxes"]) < 120          # one image truncated, one not
    for g, (wb, wsc) in zip(got, want):
        assert np.array_equal(g["logits"], wsc)
        assert g["boxes"].shape == wb.shape and np.abs(g["boxes"] - wb).max() <= 2 * C.EPS32 * 68
        assert g["counters"][:, 3].sum() > 0.2 * g["counters"][:, 0].sum()          # the NMS did suppress


def test_the_base_case_is_what_the_gpu_tests_need():
    case = C.BASE
    cells = C.base_cells()
    logits, deltas = C.base_inputs()
    res = C.proposals_np(logits, deltas, cells, case["strides"], case["image_sizes"], case["thresh"], case["pre"], case["post"],
                         case["min_box"])
    counters = np.stack([r["counters"] for r in res])
    assert counters[0, :, 0].tolist() == [600, 600, 420, 105, 36]                    # p2 and p3 select, p4..p6 take everything
    cand, supp = counters[:, :, 0].sum(), counters[:, :, 3].sum()
    assert 0.2 * cand <= supp <= 0.95 * cand
    kept = counters[:, :, 4].sum(axis=1)
    assert (kept > case["post"]).any() and (kept < case["post"]).any()             # truncated and not truncated
    assert [len(r["boxes"]) for r in res] == [min(int(k), case["post"]) for k in kept]
    undecided = total = 0
    for n, (h, w) in enumerate(case["image_sizes"]):
        for _, _, raw64 in C.candidates_np(logits, deltas, cells, case["strides"], n, case["pre"], dtype=np.float64):
            undecided += int(C.undecided_rows(raw64, h, w, case["min_box"]).sum())
            total += len(raw64)
    assert undecided <= 0.01 * total


# ---------------------------------------------------------------------------------------------------------------- host checks
def _args(N=2, A=3, maps=((4, 5), (2, 3)), dtype=torch.float32):
    logits = [torch.zeros((N, A, h, w), dtype=dtype) for h, w in maps]
    deltas = [torch.zeros((N, 4 * A, h, w), dtype=dtype) for h, w in maps]
    cells = rpn.cell_anchors([[32], [64]][:len(maps)], [0.5, 1.0, 2.0][:A])
    return logits, deltas, cells, [4, 8][:len(maps)], [(16, 20)] * N


KW = {"nms_thresh": 0.7, "pre_nms_topk": 100, "post_nms_topk": 50}


def test_abi_exports():
    assert {"umr_rpn_workspace", "umr_rpn_proposals"} <= set(L.exported_symbols())
    assert L.RESTYPES["umr_rpn_workspace"] is L._i64 and "umr_rpn_proposals" not in L.RESTYPES
    assert len(L.ARGTYPES["umr_rpn_proposals"]) == 29 and L.ARGTYPES["umr_rpn_proposals"][9:16] == [L.ctypes.c_float] * 6 + [L.ctypes.c_double]
    assert rpn.MAX_PRE_NMS_TOPK == 4096 and rpn.MAX_ANCHORS == 16 and rpn.MAX_LEVELS == 8 and rpn.SELECT_SHARE == 16384
    src = open(L.os.path.join(L.CSRC, "rpn.hip")).read()
    assert "RPN_SELECT_SHARE = 16384" in src and "RPN_MAX_K = 4096" in src and "RPN_MAX_A = 16" in src


def test_cpu_tensors_raise_runtime_error():
    lg, dl, cells, strides, sizes = _args()
    with pytest.raises(RuntimeError, match="MI355X only"):
        rpn.rpn_proposals(lg, dl, cells, strides, sizes, **KW)


def _raises(match, mutate, **kw):
    lg, dl, cells, strides, sizes = _args()
    a = {"lg": lg, "dl": dl, "cells": cells, "strides": strides, "sizes": sizes}
    mutate(a)
    with pytest.raises(ValueError, match="rpn: .*" + match):
        rpn.rpn_proposals(a["lg"], a["dl"], a["cells"], a["strides"], a["sizes"], **{**KW, **kw})


def test_value_errors_before_any_launch():
    _raises("one tensor per level", lambda a: a.update(dl=a["dl"][:1]))
    _raises("one tensor per level", lambda a: a.update(lg=[], dl=[]))
    _raises("levels of cell anchors", lambda a: a.update(cells=a["cells"][:1]))
    _raises("between 1 and 8 levels", lambda a: a.update(cells=list(a["cells"]) * 5))
    _raises(r"cells\[1\] must be float32", lambda a: a.update(cells=[a["cells"][0], a["cells"][1].double()]))
    _raises("the same A on every level", lambda a: a.update(cells=[a["cells"][0], a["cells"][1][:2]]))
    _raises("1 <= A <= 16", lambda a: a.update(cells=[torch.zeros((17, 4))] * 2))
    _raises("strides for 2 levels", lambda a: a.update(strides=[4]))
    _raises(r"strides\[1\] must be an integer", lambda a: a.update(strides=[4, 0]))
    _raises(r"strides\[0\] must be an integer", lambda a: a.update(strides=[4.0, 8]))
    _raises(r"pred_anchor_deltas\[0\] must be float32 or bfloat16", lambda a: a["dl"].__setitem__(0, a["dl"][0].double()))
    _raises(r"pred_objectness_logits\[1\] must be float32 or bfloat16", lambda a: a["lg"].__setitem__(1, a["lg"][1][0]))
    _raises("one type for all", lambda a: a["dl"].__setitem__(1, a["dl"][1].bfloat16()))
    _raises("not contiguous", lambda a: a["lg"].__setitem__(0, a["lg"][0].transpose(2, 3).contiguous().transpose(2, 3)))
    _raises("level 1: logits", lambda a: a["dl"].__setitem__(1, a["dl"][1][:, :8].contiguous()))
    _raises("level 0: logits", lambda a: a["lg"].__setitem__(0, a["lg"][0][:1].contiguous()))
    _raises("image sizes for 2 images", lambda a: a.update(sizes=[(16, 20)]))
    _raises(r"image_sizes\[1\] must be \(h, w\)", lambda a: a.update(sizes=[(16, 20), 7]))
    _raises(r"image_sizes\[0\] must be finite", lambda a: a.update(sizes=[(float("inf"), 20), (16, 20)]))
    _raises("nms_thresh is NaN", lambda a: None, nms_thresh=float("nan"))
    _raises("min_box_size must be a number", lambda a: None, min_box_size="x")
    _raises(r"pre_nms_topk must be an integer in \[1, 4096\]", lambda a: None, pre_nms_topk=4097)
    _raises(r"pre_nms_topk must be an integer in \[1, 4096\]", lambda a: None, pre_nms_topk=0)
    _raises("post_nms_topk must be an integer >= 1", lambda a: None, post_nms_topk=0)
    _raises("post_nms_topk must be an integer", lambda a: None, post_nms_topk=True)
    _raises("box2box_weights", lambda a: None, box2box_weights=(1, 1, 1))
    _raises("box2box_weights", lambda a: None, box2box_weights=(1, 1, 0, 1))
    _raises(r"offset must lie in \[0, 1\)", lambda a: None, offset=1.0)
    _raises(r"offset must lie in \[0, 1\)", lambda a: None, offset=-0.25)
    _raises("not exactly representable", lambda a: None, offset=0.1)
    _raises("not exactly representable", lambda a: a.update(strides=[4, 3]), offset=float(F32(1) / F32(3)))


def test_value_errors_of_sizes_that_need_no_memory():
    """shapes at the limits, as meta tensors: the checks read shapes and types only"""
    def meta(*shape):
        return torch.empty(shape, dtype=torch.float32, device="meta")
    cells = rpn.cell_anchors([[32]], [0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match=r"rpn: level 0: H \* W \* A = 3221225472, 2\^31 or more"):
        rpn.rpn_proposals([meta(1, 3, 1 << 15, 1 << 15)], [meta(1, 12, 1 << 15, 1 << 15)], cells, [1], [(8, 8)], **KW)
    with pytest.raises(ValueError, match=r"rpn: level 0: H \* stride and W \* stride must be at most 2\^24"):
        rpn.rpn_proposals([meta(1, 3, 4, 4)], [meta(1, 12, 4, 4)], cells, [1 << 23], [(8, 8)], **KW)
    with pytest.raises(ValueError, match="rpn: 8192 images x 8 levels: at most 65535"):
        rpn.rpn_proposals([meta(8192, 3, 1, 1)] * 8, [meta(8192, 12, 1, 1)] * 8, cells * 8, [4] * 8, [(8, 8)] * 8192, **KW)


def test_grid_anchor_and_cell_value_errors():
    cells = rpn.cell_anchors([[32]], [1.0])
    with pytest.raises(ValueError, match="rpn: 1 feature sizes for"):
        rpn.grid_anchors(cells * 2, [4, 8], [(2, 2)])
    with pytest.raises(ValueError, match=r"rpn: feature_sizes\[0\]"):
        rpn.grid_anchors(cells, [4], [(0, 2)])
    with pytest.raises(ValueError, match="rpn: offset"):
        rpn.grid_anchors(cells, [4], [(2, 2)], offset=-0.5)
    with pytest.raises(ValueError, match="at most 2\\^24"):
        rpn.grid_anchors(cells, [1 << 20], [(32, 2)])
    with pytest.raises(ValueError, match="rpn: level 0: sizes and aspect ratios must be positive"):
        rpn.cell_anchors([[0]], [1.0])
    with pytest.raises(ValueError, match="rpn: 2 levels of sizes and 3 of aspect ratios"):
        rpn.cell_anchors([[32], [64]], [[1.0], [1.0], [1.0]])
    with pytest.raises(ValueError, match="rpn: sizes is a sequence"):
        rpn.cell_anchors([32], [1.0])


def test_nms_restatement_on_the_constructed_blocks():
    """tests/nms_cases.py through nms_np: the chains keep [A, C], 64 duplicates leave one, two zero-area boxes stay (with flag 0: the
    device flags an empty box and never keeps it); a flagged rank suppresses nothing"""
    import nms_cases as NC
    boxes, kept = NC.constructed_boxes()
    NC.check_expected(C.nms_np(boxes, np.zeros(len(boxes), np.uint8), NC.THRESH))
    a, b, c = NC.CHAIN_IN_ONE_BLOCK
    assert C.nms_np(boxes[[a, b, c]], [0, 0, 0], NC.THRESH).tolist() == [0, 2] and C.nms_np(boxes[[b, c]], [0, 0], NC.THRESH).tolist() == [0]
    assert C.nms_np(boxes[[b, c]], [2, 0], NC.THRESH).tolist() == [1]
    assert C.nms_np(boxes[list(NC.DUPLICATES)], np.zeros(64), NC.THRESH).tolist() == [0]
    assert C.nms_np(boxes[list(NC.ZERO_AREA)], [0, 0], NC.THRESH).tolist() == [0, 1]
