"""unmore_amd.rpn on the MI355X against the restatement of tests/rpn_common.py, in layers so that a last-bit difference of expf cannot
cascade through the NMS: (1) the selected indices and logits per level are EQUAL; (2) the decoded boxes lie within
4 ulp * max(|coordinate|, frame side) of the float64 restatement (the bound tests/test_box_loss_gpu.py uses for the same arithmetic) and
the empty / non-empty flags agree wherever that bound decides them; (3) the restatement's steps 3 - 5 run on the DEVICE's decoded boxes
give the device's kept boxes, logits, order, counts and counters exactly.  Inputs whose decode is exact in float32 are compared end to
end, bit for bit."""
import numpy as np
import pytest
import torch

import rpn_common as C

pytestmark = pytest.mark.gpu

F32 = np.float32


def _dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _run(logits, deltas, cells, strides, sizes, dtype=torch.float32, **kw):
    """one call in the list form with the debug return: (per-image (boxes, logits) as NumPy, candidates dict as NumPy, counters)"""
    from unmore_amd import rpn
    dev = _dev()
    lg = [torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype) for x in logits]
    dl = [torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype) for x in deltas]
    dbg, st = {}, {}
    out = rpn.rpn_proposals(lg, dl, [torch.from_numpy(np.asarray(c, F32)) for c in cells], list(strides), list(sizes), stats=st, _debug=dbg,
                            **kw)
    assert all(b.dtype == torch.float32 and s.dtype == torch.float32 and b.is_cuda and tuple(b.shape) == (len(s), 4) for b, s in out)
    cand = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in dbg.items()}
    assert st["counters"].dtype == torch.int32 and st["counters"].is_cuda
    return [(b.cpu().numpy(), s.cpu().numpy()) for b, s in out], cand, st["counters"].cpu().numpy()


def _widen(arrays, dtype):
    """what the device reads: the float32 values of the arrays after the cast to `dtype`"""
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(torch.float32).numpy() for x in arrays]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _check_layers(got, cand, counters, logits, deltas, cells, strides, sizes, thresh, pre, post, min_box=0.0, weights=(1.0, 1.0, 1.0, 1.0),
                  offset=0.0):
    """the three layers for one call; logits / deltas are the float32 values the device read.  Returns the restatement and the number of
    undecided and of all candidates."""
    ref = C.proposals_np(logits, deltas, cells, strides, sizes, thresh, pre, post, min_box, weights, offset)
    first = cand["level_first"]
    undecided = total = 0
    worst = 0.0
    for n, (h, w) in enumerate(sizes):
        c64 = C.candidates_np(logits, deltas, cells, strides, n, pre, weights, offset, dtype=np.float64)
        lb, ls, lf = [], [], []
        for l, lev in enumerate(ref[n]["levels"]):
            sl = slice(first[l], first[l + 1])
            idx, sc, raw = cand["indices"][n, sl], cand["scores"][n, sl], cand["raw_boxes"][n, sl]
            box, flag = cand["boxes"][n, sl], cand["flags"][n, sl]
            # layer 1: equal
            assert np.array_equal(idx, lev["indices"]), (n, l)
            assert np.array_equal(_bits(sc), _bits(lev["logits"])), (n, l)
            # layer 2: within the bound of float64
            raw64 = c64[l][2]
            fin = np.isfinite(raw64).all(axis=1) & np.isfinite(raw).all(axis=1)
            assert np.array_equal(flag == 1, lev["flags"] == 1), (n, l)
            bound = 4 * C.EPS32 * np.maximum(np.abs(raw64), max(h, w))
            with np.errstate(invalid="ignore"):
                err = np.abs(raw.astype(np.float64) - raw64)
            if fin.any():
                worst = max(worst, float((err[fin] / bound[fin]).max()))
            assert (err[fin] <= bound[fin]).all(), (n, l, worst)
            assert (np.abs(box.astype(np.float64) - C.clip_np(raw64, h, w, np.float64))[fin] <= bound[fin]).all(), (n, l)
            und = C.undecided_rows(raw64, h, w, min_box) & fin
            decided = fin & ~und & (lev["flags"] != 1)
            assert np.array_equal(flag[decided], lev["flags"][decided]), (n, l)
            undecided, total = undecided + int(und.sum()), total + len(idx)
            # layer 3, first half: the clip and the flags of the device's own decoded boxes, exactly
            box3, flag3 = C.flags_np(raw, sc, h, w, min_box)
            assert np.array_equal(flag3, flag), (n, l)
            ok = flag != 1
            assert np.array_equal(_bits(box3[ok]), _bits(box[ok])), (n, l)
            lb.append(box), ls.append(sc), lf.append(flag)
        # layer 3: the NMS, the merge and the truncation on the device's boxes, exactly
        kb, ks, cnt = C.finish_np(lb, ls, lf, thresh, post)
        assert got[n][0].shape == kb.shape, (n, got[n][0].shape, kb.shape)
        assert np.array_equal(_bits(got[n][0]), _bits(kb)) and np.array_equal(_bits(got[n][1]), _bits(ks)), n
        assert np.array_equal(counters[n], cnt), (n, counters[n], cnt)
    print(f"decode: worst error {worst:.3f} of the bound 4 ulp * max(|coordinate|, frame side); {undecided} of {total} rows undecided")
    return ref, undecided, total


# ---------------------------------------------------------------------------------------------------------------- the base case
@pytest.fixture(scope="module")
def base():
    case = C.BASE
    logits, deltas = C.base_inputs()
    cells = C.base_cells()
    kw = {"nms_thresh": case["thresh"], "pre_nms_topk": case["pre"], "post_nms_topk": case["post"], "min_box_size": case["min_box"]}
    got, cand, counters = _run(logits, deltas, cells, case["strides"], case["image_sizes"], **kw)
    return {"case": case, "logits": logits, "deltas": deltas, "cells": cells, "kw": kw, "got": got, "cand": cand, "counters": counters}


def test_base_case_in_layers(base):
    case = base["case"]
    ref, undecided, total = _check_layers(base["got"], base["cand"], base["counters"], base["logits"], base["deltas"], base["cells"],
                                          case["strides"], case["image_sizes"], case["thresh"], case["pre"], case["post"], case["min_box"])
    assert undecided <= 0.01 * total
    cnt = base["counters"]
    assert cnt[0, :, 0].tolist() == [600, 600, 420, 105, 36]
    assert 0.2 * cnt[:, :, 0].sum() <= cnt[:, :, 3].sum() <= 0.95 * cnt[:, :, 0].sum()       # the NMS suppresses
    kept = cnt[:, :, 4].sum(axis=1)
    assert (kept > case["post"]).any() and (kept < case["post"]).any()                     # one image truncated, another not
    assert [len(b) for b, _ in base["got"]] == [min(int(k), case["post"]) for k in kept]
    assert all((np.diff(s) <= 0).all() for _, s in base["got"])                             # the order: descending logits


def test_padded_form_and_determinism(base):
    from unmore_amd import rpn
    case, dev = base["case"], _dev()
    lg = [torch.from_numpy(x).to(dev) for x in base["logits"]]
    dl = [torch.from_numpy(x).to(dev) for x in base["deltas"]]
    cells = [torch.from_numpy(c) for c in base["cells"]]
    runs = [rpn.rpn_proposals(lg, dl, cells, list(case["strides"]), list(case["image_sizes"]), padded=True, **base["kw"]) for _ in range(2)]
    boxes, logits, counts = runs[0]
    cap = min(case["post"], sum(base["counters"][0, :, 0]))
    assert tuple(boxes.shape) == (case["N"], cap, 4) and tuple(logits.shape) == (case["N"], cap) and counts.dtype == torch.int32
    assert boxes.is_cuda and logits.is_cuda and counts.is_cuda
    for a, b in zip(runs[0], runs[1]):                                                      # the same bytes on every run
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    for n, (gb, gs) in enumerate(base["got"]):
        k = int(counts[n])
        assert k == len(gs)
        assert np.array_equal(_bits(boxes[n, :k].cpu().numpy()), _bits(gb)) and np.array_equal(_bits(logits[n, :k].cpu().numpy()), _bits(gs))
        assert not boxes[n, k:].any() and not logits[n, k:].any()                           # zero past the count


# ---------------------------------------------------------------------------------------------------------------- exact end to end
def test_exact_decode_is_equal_bit_for_bit():
    """dw = dh = 0, dx and dy multiples of 1/8, square power-of-two cells, offset 0.5 with even strides: every decode operation is exact in
    float32 (expf(0) = 1), so nothing is layered -- every output equals the restatement's"""
    rng = np.random.RandomState(11)
    N, maps, strides = 2, ((24, 30), (12, 15), (6, 8)), (4, 8, 16)
    cells = [C.cell_anchors_np((s,), (1.0,)) for s in (16, 32, 64)]
    logits = [rng.standard_normal((N, 1, h, w)).astype(F32) for h, w in maps]
    deltas = []
    for h, w in maps:
        d = np.zeros((N, 4, h, w), F32)
        d[:, :2] = rng.randint(-6, 7, (N, 2, h, w)).astype(F32) / F32(8)
        deltas.append(d)
    sizes = [(96, 120), (70, 90)]
    got, cand, counters = _run(logits, deltas, cells, strides, sizes, nms_thresh=0.5, pre_nms_topk=500, post_nms_topk=200, offset=0.5)
    ref = C.proposals_np(logits, deltas, cells, strides, sizes, 0.5, 500, 200, offset=0.5)
    first = cand["level_first"]
    for n, r in enumerate(ref):
        assert np.array_equal(_bits(got[n][0]), _bits(r["boxes"])) and np.array_equal(_bits(got[n][1]), _bits(r["logits"])), n
        assert np.array_equal(counters[n], r["counters"])
        for l, lev in enumerate(r["levels"]):
            sl = slice(first[l], first[l + 1])
            assert np.array_equal(cand["indices"][n, sl], lev["indices"]) and np.array_equal(cand["flags"][n, sl], lev["flags"])
            assert np.array_equal(_bits(cand["raw_boxes"][n, sl]), _bits(lev["raw"])) and np.array_equal(_bits(cand["boxes"][n, sl]), _bits(lev["boxes"]))
    assert counters[:, :, 3].sum() > 0.2 * counters[:, :, 0].sum() and len(got[0][0]) == 200


# ---------------------------------------------------------------------------------------------------------------- top-k boundaries
def _one_level(rng, N, A, h, w, scale=0.2):
    return [rng.standard_normal((N, A, h, w)).astype(F32)], [(rng.standard_normal((N, 4 * A, h, w)) * scale).astype(F32)]


@pytest.mark.parametrize("hw,pre", [((64, 80), 2000), ((64, 80), 4096), ((80, 96), 2000), ((120, 140), 4096)])
def test_topk_one_large_level(hw, pre):
    """64 x 80 x 3 = 15 360 scores: one workgroup's share; 80 x 96 x 3 = 23 040 and 120 x 140 x 3 = 50 400: above rpn.SELECT_SHARE = 16 384,
    two and four partial selects whose survivors are selected again, the last part shorter than the others"""
    from unmore_amd import rpn
    n_scores = hw[0] * hw[1] * 3
    assert (n_scores > rpn.SELECT_SHARE) == (hw != (64, 80)) and n_scores % rpn.SELECT_SHARE != 0
    rng = np.random.RandomState(hw[0] + pre)
    logits, deltas = _one_level(rng, 2, 3, *hw)
    cells = [C.cell_anchors_np((32,), (0.5, 1.0, 2.0))]
    sizes = [(hw[0] * 4, hw[1] * 4), (hw[0] * 4 - 37, hw[1] * 4 - 51)]
    got, cand, counters = _run(logits, deltas, cells, (4,), sizes, nms_thresh=0.65, pre_nms_topk=pre, post_nms_topk=1000)
    _check_layers(got, cand, counters, logits, deltas, cells, (4,), sizes, 0.65, pre, 1000)
    assert counters[:, 0, 0].tolist() == [pre, pre]


@pytest.mark.parametrize("hw", [(40, 50), (80, 96)])
def test_topk_with_the_kth_value_tied_hundreds_of_times(hw):
    """logits drawn from 16 distinct values: the k-th value is shared by hundreds of scores and the lower f wins, within one select and
    across the partial selects"""
    rng = np.random.RandomState(21)
    logits, deltas = _one_level(rng, 2, 3, *hw)
    logits = [(rng.randint(0, 16, logits[0].shape).astype(F32) - F32(8)) * F32(0.25)]
    cells = [C.cell_anchors_np((32,), (0.5, 1.0, 2.0))]
    sizes = [(hw[0] * 4, hw[1] * 4)] * 2
    pre = 1000
    flat = C.flat_scores(logits[0][0])
    kth = np.sort(flat)[::-1][pre - 1]
    assert (flat == kth).sum() > 200 and (flat > kth).sum() < pre < (flat >= kth).sum()     # the cut falls inside a run of equal values
    got, cand, counters = _run(logits, deltas, cells, (4,), sizes, nms_thresh=0.65, pre_nms_topk=pre, post_nms_topk=400)
    _check_layers(got, cand, counters, logits, deltas, cells, (4,), sizes, 0.65, pre, 400)


def test_topk_special_values_at_inference():
    """fewer anchors than k on the second level; +-inf, +-0.0 and NaN logits, a NaN and an inf delta: dropped and counted, never raised"""
    rng = np.random.RandomState(31)
    N, A, maps, strides = 2, 3, ((12, 16), (5, 7)), (8, 16)
    logits = [rng.standard_normal((N, A, h, w)).astype(F32) for h, w in maps]
    deltas = [(rng.standard_normal((N, 4 * A, h, w)) * 0.2).astype(F32) for h, w in maps]
    z = logits[0]
    z[0, 0, 0, :4] = [np.nan, np.inf, -np.inf, np.nan]
    z[0, 1, 3, :6] = [0.0, -0.0, 0.0, -0.0, -0.0, 0.0]
    z[0, 2, 5, 5:9] = 5.0                                             # finite ties at the top
    z[1] -= F32(1.5)                                                  # few scores above the zeros: the zeros are selected
    z[1, :, 2, :] = 0.0
    z[1, 1, 2, ::2] = -0.0
    logits[1][1, 0, 0, 0], logits[1][1, 2, 4, 6] = np.nan, -np.inf    # every anchor of this level is taken: the -inf too
    deltas[0][0, 2 * 4 + 2, 5, 6] = np.nan                            # dw of a top candidate
    deltas[0][0, 2 * 4 + 0, 5, 7] = np.inf
    deltas[0][0, 2 * 4 + 3, 5, 8] = np.inf                            # dh = +inf is clamped: still finite
    cells = [C.cell_anchors_np((s,), (0.5, 1.0, 2.0)) for s in (32, 64)]
    sizes = [(96, 128), (90, 100)]
    pre = 200
    assert maps[1][0] * maps[1][1] * A < pre
    got, cand, counters = _run(logits, deltas, cells, strides, sizes, nms_thresh=0.65, pre_nms_topk=pre, post_nms_topk=150)
    ref, _, _ = _check_layers(got, cand, counters, logits, deltas, cells, strides, sizes, 0.65, pre, 150)
    assert counters[:, :, 0].tolist() == [[200, 105], [200, 105]]
    assert counters[0, 0, 1] == 5 and counters[1, 1, 1] == 2 and counters[:, :, 1].sum() == 7     # NaN, NaN, +inf logits; NaN, inf deltas
    assert cand["indices"][0, :3].tolist() == [0, 9, 3]               # the NaNs first (by f), then +inf
    assert all(np.isfinite(b).all() and np.isfinite(s).all() for b, s in got)
    # the run of zeros of either sign is ordered by f alone
    zero = np.flatnonzero(cand["scores"][1, :200] == 0)
    assert len(zero) > 10 and (np.diff(cand["indices"][1, zero]) > 0).all() and np.signbit(cand["scores"][1, zero]).any()


def test_bfloat16_inputs_are_widened():
    case = C.BASE
    logits, deltas = C.base_inputs(seed=5)
    cells = C.base_cells()
    wl, wd = _widen(logits, torch.bfloat16), _widen(deltas, torch.bfloat16)
    assert not np.array_equal(wl[0], logits[0])
    got, cand, counters = _run(logits, deltas, cells, case["strides"], case["image_sizes"], dtype=torch.bfloat16, nms_thresh=case["thresh"],
                               pre_nms_topk=case["pre"], post_nms_topk=case["post"])
    _, undecided, total = _check_layers(got, cand, counters, wl, wd, cells, case["strides"], case["image_sizes"], case["thresh"], case["pre"],
                                        case["post"])
    assert undecided <= 0.01 * total
    # bfloat16 logits tie often: the cut of p2's 600 of 6720 falls inside a run of equal values in at least one image
    assert any((C.flat_scores(wl[0][n]) == cand["scores"][n, 599]).sum() > 1 for n in range(case["N"]))


# ---------------------------------------------------------------------------------------------------------------- NMS boundaries
@pytest.mark.parametrize("hw", [(7, 9), (8, 8), (5, 13), (40, 50), (64, 64)])
def test_nms_candidate_counts(hw):
    """63, 64, 65, 2000 and 4096 candidates on one level (A = 1, N = 1, one level only): around the 64-rank tiles of the suppression
    matrix and the one-word-per-lane limit of the scan"""
    n_cand = hw[0] * hw[1]
    assert n_cand in (63, 64, 65, 2000, 4096)
    rng = np.random.RandomState(n_cand)
    logits, deltas = _one_level(rng, 1, 1, *hw, scale=0.3)
    cells = [C.cell_anchors_np((24,), (1.0,))]
    sizes = [(hw[0] * 4, hw[1] * 4)]
    got, cand, counters = _run(logits, deltas, cells, (4,), sizes, nms_thresh=0.5, pre_nms_topk=4096, post_nms_topk=4096)
    _check_layers(got, cand, counters, logits, deltas, cells, (4,), sizes, 0.5, 4096, 4096)
    assert counters[0, 0, 0] == n_cand and counters[0, 0, 3] > 0.2 * n_cand and counters[0, 0, 4] == len(got[0][1]) > 0


def _line_level(q, lowered=()):
    """One level (N = 1, A = 1, H = 1, W = len(q), stride 4, a 64 x 64 cell anchor) whose candidate of rank r decodes exactly to the box
    (q[r], 0, q[r] + 64, 32) of tests/nms_cases.py: logit len(q) - x makes position x rank x; dw = dh = 0 and dx = (q + 32 - 4 x) / 64, a
    multiple of 1/64, keep every operation of the decode exact; the frame (64, 65536) clips y1 = -32 to 0 and nothing else.  The ranks in
    `lowered` get dy = -12 / 64: rows -44 .. 20, 20 high after the clip."""
    K = len(q)
    logits = [np.arange(K, 0, -1, dtype=F32).reshape(1, 1, 1, K)]
    d = np.zeros((1, 4, 1, K), F32)
    d[0, 0, 0] = (np.asarray(q, np.float64) + 32 - 4 * np.arange(K)) / 64
    d[0, 1, 0, list(lowered)] = -12 / 64
    return logits, [d], [C.cell_anchors_np((64,), (1.0,))], (4,), [(64, 65536)]


def test_nms_on_the_constructed_blocks():
    """tests/nms_cases.py as one level's candidates: chains inside a 64-rank block, into the next and over a wholly suppressed one, and a
    block of duplicates.  The zero-area pair is left out: a box of no width is flagged empty here and never reaches the scan as valid."""
    import nms_cases as NC
    q, width, kept = NC.constructed(zero_area=False)
    logits, deltas, cells, strides, sizes = _line_level(q)
    kw = {"nms_thresh": NC.THRESH, "pre_nms_topk": 4096, "post_nms_topk": 4096}
    got, cand, counters = _run(logits, deltas, cells, strides, sizes, **kw)
    _check_layers(got, cand, counters, logits, deltas, cells, strides, sizes, NC.THRESH, 4096, 4096)
    assert np.array_equal(_bits(cand["boxes"][0]), _bits(NC.line_boxes(q)))               # the decode is exact
    assert np.array_equal(_bits(got[0][0]), _bits(NC.line_boxes(q)[kept]))
    assert counters[0, 0].tolist() == [len(q), 0, 0, len(q) - len(kept), len(kept)]


def test_nms_starts_from_the_valid_set():
    """K = 65, the last valid word holds one rank.  Rank 30 is flagged empty (20 high, min_box_size 24) and lies on rank 50 with IoU
    20 / 32: its row of the matrix has rank 50's bit, and rank 50 is kept because an invalid rank suppresses nothing.  Ranks 62, 63, 64
    are a chain over the word boundary: 63 goes, 64 -- the partial word's only rank -- stays."""
    import nms_cases as NC
    q = 1000 + 128 * np.arange(65)
    q[30] = q[50] = 0
    q[62], q[63], q[64] = 200, 216, 232
    logits, deltas, cells, strides, sizes = _line_level(q, lowered=(30,))
    kw = {"nms_thresh": NC.THRESH, "pre_nms_topk": 4096, "post_nms_topk": 4096, "min_box_size": 24.0}
    got, cand, counters = _run(logits, deltas, cells, strides, sizes, **kw)
    _check_layers(got, cand, counters, logits, deltas, cells, strides, sizes, NC.THRESH, 4096, 4096, min_box=24.0)
    assert cand["flags"][0].tolist() == [2 if r == 30 else 0 for r in range(65)]
    assert cand["boxes"][0, 30].tolist() == [0, 0, 64, 20] and C.iou_row(cand["boxes"][0, 30], cand["boxes"][0, 50])[0] > NC.THRESH
    kept = [r for r in range(65) if r not in (30, 63)]
    assert np.array_equal(_bits(got[0][0]), _bits(NC.line_boxes(q)[kept]))
    assert counters[0, 0].tolist() == [65, 0, 1, 1, 63]


def test_an_image_without_a_box_left():
    """every dx of the second image is 40 anchor widths to the right: all of its boxes clip to zero width, its count is 0 and its views
    are empty"""
    rng = np.random.RandomState(41)
    logits, deltas = _one_level(rng, 2, 3, 6, 8)
    deltas[0][1, 0::4] = 40.0
    cells = [C.cell_anchors_np((32,), (0.5, 1.0, 2.0))]
    sizes = [(48, 64), (48, 64)]
    got, cand, counters = _run(logits, deltas, cells, (8,), sizes, nms_thresh=0.65, pre_nms_topk=100, post_nms_topk=50)
    _check_layers(got, cand, counters, logits, deltas, cells, (8,), sizes, 0.65, 100, 50)
    assert got[1][0].shape == (0, 4) and got[1][1].shape == (0,) and counters[1, 0].tolist() == [100, 0, 100, 0, 0] and len(got[0][1]) > 0


# ---------------------------------------------------------------------------------------------------------------- raises
def test_training_raises_on_a_non_finite_candidate():
    from unmore_amd import rpn
    rng = np.random.RandomState(51)
    logits, deltas = _one_level(rng, 2, 3, 6, 8)
    logits[0][1, 0, 2, 3] = 50.0
    deltas[0][1, 0, 2, 3] = np.nan                                    # the top candidate of image 1
    dev = _dev()
    lg, dl = [torch.from_numpy(logits[0]).to(dev)], [torch.from_numpy(deltas[0]).to(dev)]
    cells = [torch.from_numpy(C.cell_anchors_np((32,), (0.5, 1.0, 2.0)))]
    kw = {"nms_thresh": 0.65, "pre_nms_topk": 100, "post_nms_topk": 50}
    with pytest.raises(FloatingPointError, match="Predicted boxes or scores contain Inf/NaN. Training has diverged."):
        rpn.rpn_proposals(lg, dl, cells, [8], [(48, 64)] * 2, training=True, **kw)
    st = {}
    out = rpn.rpn_proposals(lg, dl, cells, [8], [(48, 64)] * 2, training=False, stats=st, **kw)        # inference: dropped and counted
    assert st["counters"][:, 0, 1].tolist() == [0, 1] and all(torch.isfinite(b).all() for b, _ in out)
    boxes, _, counts = rpn.rpn_proposals(lg, dl, cells, [8], [(48, 64)] * 2, training=True, padded=True, **kw)    # no host read, no raise
    assert counts.tolist() == [len(out[0][1]), len(out[1][1])] and torch.isfinite(boxes).all()
    dl[0][1, 0, 2, 3] = 0.0
    assert len(rpn.rpn_proposals(lg, dl, cells, [8], [(48, 64)] * 2, training=True, **kw)) == 2


# ---------------------------------------------------------------------------------------------------------------- chaining
def test_outputs_feed_the_pooler_and_the_inference_tail(base):
    """the list form's views go into roi_pool.assign_boxes_to_levels and detector_inference.fast_rcnn_inference as they are"""
    from det_post_common import select_numpy
    from roi_pool_common import assign_levels
    from unmore_amd import detector_inference, roi_pool, rpn
    case, dev = base["case"], _dev()
    lg = [torch.from_numpy(x).to(dev) for x in base["logits"]]
    dl = [torch.from_numpy(x).to(dev) for x in base["deltas"]]
    props = rpn.rpn_proposals(lg, dl, [torch.from_numpy(c) for c in base["cells"]], list(case["strides"]), list(case["image_sizes"]),
                              **base["kw"])
    levels = roi_pool.assign_boxes_to_levels([b for b, _ in props], 2, 5)
    boxes_np = np.concatenate([b.cpu().numpy() for b, _ in props])
    assert levels.dtype == torch.int64 and tuple(levels.shape) == (len(boxes_np),)
    assert (levels.cpu().numpy() == assign_levels(boxes_np, 2, 5)).mean() >= 0.99          # test_roi_pool_gpu.py pins the rule itself
    assert len(set(levels.tolist())) > 1
    scores = [torch.stack((torch.sigmoid(s), 1 - torch.sigmoid(s)), dim=1) for _, s in props]
    items, kept = detector_inference.fast_rcnn_inference([b for b, _ in props], scores, list(case["image_sizes"]), 0.05, 0.5, 100)
    for n, (item, rows) in enumerate(zip(items, kept)):
        wb, ws, _, wr = select_numpy(props[n][0].cpu().numpy(), scores[n].cpu().numpy(), case["image_sizes"][n], 0.05, 0.5, 100)
        assert np.array_equal(item["pred_boxes"].cpu().numpy(), wb) and np.array_equal(item["scores"].cpu().numpy(), ws)
        assert np.array_equal(rows.cpu().numpy(), wr) and 0 < len(wr) < len(props[n][1])
